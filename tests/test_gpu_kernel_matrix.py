"""Every kernel of parallax_amd/csrc/cotix_plan.h on the GPU, one test per row
of the ledger (tests/kernel_matrix.py; tests/test_kernel_matrix_cpu.py proves
on CPU that the rows' kernels are the kernel list).  Each test re-plans its
row with the device's own inputs and asserts the kernel is still the row's,
runs the row through the library with guarded output buffers, and compares
every output with the case's reference (the torch VJP oracles at the cases'
tolerances, returns and rewards bit for bit, the C port bit for bit for the
step rows) and with the host emulation of the same row bit for bit."""
import numpy as np
import pytest

import kernel_matrix as KM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def replan(torch, row):
    """The row's launches planned with this device's compute units and the
    COTIX_KEY_HELPER / COTIX_SPLIT_BWD settings the library reads: still the
    row's kernels.  A machine whose settings rule a kernel out fails the row."""
    L = KM.libs()
    dev = KM.device_inputs(torch)
    h = KM.plan_scene(L.emu, L.g, row)
    for launch, key in row.keys:
        p = KM.plan(L.g, h, row, launch, **dev)
        assert p["ew"] == row.ew and KM.plan_key(p) == key, (row.id, launch, dev, p)


def same_as_emulation(row, got, names):
    want = KM.emu_row(row)
    for k in names:
        if k in want or k in got:
            assert KM.same_bits(got[k], want[k]), "%s: %s != the host emulation's" % (row.id, k)


@pytest.mark.parametrize("row", KM.ROWS, ids=KM.IDS)
def test_row(torch_cuda, row):
    torch = torch_cuda
    replan(torch, row)
    if row.kind == "rollout":
        got = KM.gpu_rollout(torch, row)
        KM.check_rollout(row, got, "matrix_gpu")
        same_as_emulation(row, got, ["ret", "dyn", "keys", "err"] + [
            "%s:%s" % (w, n) for n in KM.launches(row) for w in ("ga", "gd", "gp", "gg")])
    elif row.kind == "eval":
        got = KM.gpu_eval(torch, row)
        KM.check_eval(row, got, "matrix_gpu")
        same_as_emulation(row, got, ["dyn", "keys", "err", "reward", "finished", "rec", "gc", "gd", "gv"] + [
            k + ":eval" for k in ("dyn", "keys", "err", "reward", "finished")])
        for k in ("gc", "gd", "gv"):  # every word of the batch written
            assert not np.any(got[k] == KM.SENTINEL_F), k
    else:
        got, form = KM.gpu_step(torch, row)
        assert form == KM.step_form(row), "%s: cotix_scene_last_step_form %d" % (row.id, form)
        KM.check_step(row, got)
        same_as_emulation(row, got, ["dyn", "keys", "err"])
