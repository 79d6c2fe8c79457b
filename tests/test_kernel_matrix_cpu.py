"""The kernel ledger (tests/kernel_matrix.py) on CPU: every row's launches plan
exactly the kernels the row claims, the rows' kernels are the kernel list of
parallax_amd/csrc/cotix_plan.h -- no entry without a row, no row without an
entry --, and every row runs on the host emulation and meets its case's
reference: the torch VJP oracles at the cases' tolerances (returns and rewards
bit for bit), the C port of the oracle bit for bit for the step rows, and the
tilings of a case bit-identical to each other.  tests/test_gpu_kernel_matrix.py
runs the same rows on the GPU."""
import collections

import numpy as np
import pytest

import kernel_matrix as KM

# The rows the ledger must hold, written out: a row that is deleted fails
# test_ledger_is_closed even where another row runs the same kernels (the
# cases differ: the circle x polygon VJP, per-env geometry rows).
EXPECTED_IDS = (
    ["rollout-%s-ew%d" % (c, e) for c in ("box5x16", "lunar4x8") for e in (1, 2, 4, 8)]
    + ["rollout-%s-ew%d" % (c, e) for c in ("ball_poly4x8", "lunar_penv4x8") for e in (2, 8)]
    + ["eval-%s-ew%d" % (c, e) for c in ("piecewise", "lunar") for e in (1, 2, 4, 8)]
    + ["step-%s-ew%d" % (c, e) for c in ("robocup_cp", "convex", "aabb_poly", "circle_poly") for e in (1, 2, 4, 8)]
    + ["step-%s-ew%d-spec" % (c, e) for c in ("robocup", "robocup_part", "lunar", "lunar_part") for e in (2, 4)]
    + ["step-box-ew4-spec", "rollout-box5x16-ew4-spec", "rollout-robocup6x6-ew4-spec", "eval-piecewise-ew4-spec",
       "eval-goal-ew4-spec", "help-l1-robocup-ew4", "help-robocup-ew4", "split-robocup16x8-ew4"])


@pytest.fixture(scope="module")
def L():
    return KM.libs()


@pytest.mark.parametrize("row", KM.ROWS, ids=KM.IDS)
def test_ledger_is_exact(L, row):
    """plan_launch picks exactly the row's key for every launch of the row,
    with the helper and split forms enabled, whether or not the device's CU
    count is known (where the row does not depend on it)."""
    h = KM.plan_scene(L.emu, L.g, row)
    for launch, key in row.keys:
        for cus in ((256, 0) if row.cus_free else (256, 1, 304)):
            p = KM.plan(L.g, h, row, launch, cus=cus)
            assert p["ew"] == row.ew and KM.plan_key(p) == key, (row.id, launch, cus, p)
    if row.kind == "step":  # what cotix_scene_last_step_form reports
        assert KM.plan(L.g, h, row, "step")["family"] == KM.step_form(row)


def test_ledger_is_closed(L):
    """The union of the rows' kernels is the kernel list: a kernel added to
    cotix_plan.h without a row fails here, and so does a row whose kernel is
    not (or no longer) in the list."""
    assert sorted(KM.IDS) == sorted(EXPECTED_IDS)
    listed = KM.kernel_list(L.g)
    rows = set().union(*[KM.row_keys(r) for r in KM.ROWS])
    assert not listed - rows, "kernels without a ledger row: %s" % sorted(listed - rows)
    assert not rows - listed, "ledger rows of kernels that are not listed: %s" % sorted(rows - listed)
    # the list as the issue counts it: 24 generic programs at 4 tilings, the
    # specializations, two helper forms and one split form
    n = collections.Counter((k[0], k[0] == "step" and k[3] == KM.GENERIC) for k, _ in listed)
    assert n[("step", True)] == 24 * 4 and n[("help", False)] == 2 and n[("split", False)] == 1
    assert len(listed) == 96 + n[("step", False)] + 3
    # every other emulation library carries the same list
    assert KM.kernel_list(L.p) == listed and KM.kernel_list(L.e) == listed


@pytest.mark.parametrize("row", KM.ROWS, ids=KM.IDS)
def test_row_on_the_emulation_meets_its_reference(row):
    out = KM.emu_row(row)
    if row.kind == "rollout":
        KM.check_rollout(row, out, "matrix")
    elif row.kind == "eval":
        KM.check_eval(row, out, "matrix")
    else:
        KM.check_step(row, out)


GROUPS = collections.defaultdict(list)
for _r in KM.ROWS:
    GROUPS[(_r.kind, _r.case, _r.envs, _r.B, _r.n_steps, _r.stages)].append(_r)
GROUPS = {"-".join([k[0], k[1]]): v for k, v in GROUPS.items() if len(v) > 1}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tilings_are_bit_identical(group):
    """Every tiling (and specialization) of a case gives the same bits."""
    rows = GROUPS[group]
    ref = KM.emu_row(rows[0])
    for r in rows[1:]:
        got = KM.emu_row(r)
        for k in ref:
            if isinstance(ref[k], np.ndarray) and k in got and k not in ("sd", "sk", "tape", "geom"):
                assert KM.same_bits(ref[k], got[k]), (rows[0].id, r.id, k)
