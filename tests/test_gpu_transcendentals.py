"""sincos32 / atan2_32 on the device, against float64 and the host copies.

tests/test_transcendentals_cpu.py holds the three host copies of the kernels
(Python oracle, C port, the kernels' code on the host) to float64 and to one
another; here the gfx950 code is held to the same bounds and to the host
emulation bit for bit, through the paths that call it: cotix_render (phase
T's forward_vector arithmetic), cotix_order_clockwise, the fused step kernel
at every tiling, and the rollout backward.  Inputs:
tests/transcendental_probes.py (every binade, multiples of pi/2 across the
8192 seam, 6.6e6, 2^31 * pi/2, FLT_MAX).

Maxima measured on the MI355X: sin/cos 7.08e-8 (bit-identical to the host's),
|s^2 + c^2 - 1| 1.15e-7, rendered edge lengths 3.0e-7 relative at angles up
to 1e20."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import transcendental_probes as TP  # noqa: E402
from test_gpu_parity import _pa_bodies, diff_report, same_f32, torch_cuda, u32_to_i32  # noqa: E402,F401

F = np.float32


@pytest.fixture(scope="module")
def emu_lib():
    """The kernels' code on the host: built when missing, never a skip."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "build/libcotix_emu.so"], check=True)
    import emu
    return emu, emu.load()


@pytest.fixture(scope="module")
def cport_lib():
    from cotix_oracle import cport
    assert os.path.exists(cport.LIB), "oracle C port %s missing (python __graft_entry__.py, or make -C oracle)" % cport.LIB
    return cport, cport.load()


def _world(pa, torch, bodies, B, keys=None):
    k = None if keys is None else torch.tensor(u32_to_i32(keys), device="cuda")
    return pa.World(_pa_bodies(pa, bodies), B, "cuda", k)


def test_sincos_on_device(torch_cuda, emu_lib):
    """One cotix_render of the probe triangle, one env per probe: the device's
    (sin, cos) of every probe == the host emulation's sincos32 bit for bit (up
    to the sign of a zero, which c * 1 + (-s) * 0 does not keep), within 2^-23
    of float64's and within 2^-22 of the unit circle; +-inf and NaN give NaN."""
    torch = torch_cuda
    import parallax_amd as pa
    from parallax_amd import render as R
    emu, lib = emu_lib
    x = np.ascontiguousarray(TP.PROBES)
    w = _world(pa, torch, TP.probe_triangle_bodies(), x.size)
    w.set_dyn(torch.tensor(TP.probe_dyn(x), device="cuda"))
    prims = R.render(w).cpu().numpy()
    assert prims.shape == (x.size, 3, 4)
    s, c = TP.sincos_from_triangle(prims)
    ws, wc = np.zeros_like(x), np.zeros_like(x)
    lib.emu_sincos(x.ctypes.data_as(emu.P_), x.size, ws.ctypes.data_as(emu.P_), wc.ctypes.data_as(emu.P_))
    assert same_f32(s + F(0), ws + F(0)), diff_report(s + F(0), ws + F(0))
    assert same_f32(c + F(0), wc + F(0)), diff_report(c + F(0), wc + F(0))
    fin = np.isfinite(x)
    assert np.isnan(s[~fin]).all() and np.isnan(c[~fin]).all()
    xf, sf, cf = x[fin].astype(np.float64), s[fin].astype(np.float64), c[fin].astype(np.float64)
    es, ec, eu = np.abs(sf - np.sin(xf)), np.abs(cf - np.cos(xf)), np.abs(sf * sf + cf * cf - 1.0)
    print("device: max |sin err| %.3g, |cos err| %.3g, |s2+c2-1| %.3g over %d probes"
          % (np.nanmax(es), np.nanmax(ec), np.nanmax(eu), xf.size))
    assert not np.isnan(es).any() and not np.isnan(ec).any()
    k = int(np.argmax(np.maximum(es, ec)))
    assert max(es.max(), ec.max()) <= TP.SINCOS_TOL, (xf[k], sf[k], cf[k])
    assert eu.max() <= TP.UNIT_TOL, xf[int(np.argmax(eu))]


def test_order_clockwise_on_device_vs_float64(torch_cuda):
    """cotix_order_clockwise of 3-, 4-, 6- and 8-gons of scale 2^-60 .. 2^60
    about a far-off mean, some vertices next to an axis: the float64 arctan2
    order (unambiguous: every gap above 1e-3 rad, see clockwise_cases) and the
    oracle's."""
    torch = torch_cuda
    import parallax_amd as pa
    from cotix_oracle import geometry as G
    for nv in (3, 4, 6, 8):
        v, order = TP.clockwise_cases(nv)
        want = np.stack([p[o] for p, o in zip(v, order)])
        t = torch.tensor(v, device="cuda")
        pa._ffi.check(pa._ffi.lib.cotix_order_clockwise(pa._ffi.ptr(t), v.shape[0], nv, pa._ffi.stream_ptr()), "ocw")
        got = t.cpu().numpy()
        assert same_f32(got, want), (nv, diff_report(got, want))
        orc = np.array([G.order_clockwise([tuple(q) for q in p]) for p in v], F)
        assert same_f32(got, orc), (nv, diff_report(got, orc))


@pytest.mark.parametrize("scene", ["poly_box", "mixed_circle"])
def test_fused_step_at_large_angles(torch_cuda, cport_lib, scene):
    """17 fused steps, at every envs-per-wave tiling, of 16 envs whose bodies
    start at angles 8191.9 .. 1e20 of both signs (those next to 8192 cross the
    seam, both ways): state, keys, error bits and every collider choice == the
    C port bit for bit, and cotix_render of the result keeps every polygon's
    local edge lengths within 4 * 2^-23 relative: the rotation is orthonormal.
    (With the three-constant reduction alone the rows from 7e6 on missed that
    by orders of magnitude.)  No angle reduced modulo 2 pi in float64 is a
    float32, so there is no exactly reduced run to compare the choices with."""
    torch = torch_cuda
    import parallax_amd as pa
    from parallax_amd import render as R
    cport, lib = cport_lib
    bodies, dyn0, keys0, dynamic = TP.large_angle_case(scene)
    B, T = dyn0.shape[2], 17
    wd, wk, we = dyn0.copy(), keys0.copy(), np.zeros(B, np.uint32)
    wch, wcl = cport.Scene(lib, bodies).step_ex(wd, wk, we, T, cport.STAGES_ROBOCUP, trace=True, nthreads=1)
    assert (wcl >= 0).any()
    a0, a1 = np.abs(dyn0[dynamic, 4, :]), np.abs(wd[dynamic, 4, :])
    assert ((a0 < 8192) & (a1 > 8192)).sum() >= 2 and ((a0 > 8192) & (a1 <= 8192)).sum() >= 2
    for ew in (1, 2, 4, 8):
        w = _world(pa, torch, bodies, B, keys0)
        w.set_variant(ew)
        assert w.scene.variant()["envs_per_wave"] == ew
        w.set_dyn(torch.tensor(dyn0, device="cuda"))
        trc = {}
        w.step(T, 1e-2, pa._ffi.STAGES_ROBOCUP, trace=trc)
        torch.cuda.synchronize()
        got = w.dyn.cpu().numpy()
        assert same_f32(got, wd), (ew, diff_report(got, wd))
        assert np.array_equal(w.keys.cpu().numpy().view(np.uint32), wk), ew
        assert np.array_equal(w.err.cpu().numpy().view(np.uint32), we), ew
        assert np.array_equal(trc["chosen"].cpu().numpy(), wch), ew
        assert np.array_equal(trc["cells"].cpu().numpy(), wcl), ew
    prims = R.render(w).cpu().numpy()
    worst = 0.0
    for _, part, off, n in TP.polygon_part_offsets(bodies):
        want = TP.local_edge_lengths(part)
        worst = max(worst, float(np.max(np.abs(TP.rendered_edge_lengths(prims, off, n) - want) / want)))
    print("%s: max relative edge length error %.3g (bound %.3g)" % (scene, worst, 4 * 2.0 ** -23))
    assert worst <= 4 * 2.0 ** -23


def test_rollout_grad_at_large_angles_vs_oracle(torch_cuda):
    """rollout_backward of the polygon box scene started at 3.0e4 and 1.0e7
    rad against the oracle's rollout_grad, at the case's own tolerance."""
    torch = torch_cuda
    import parallax_amd as pa
    from test_gpu_parity import _check_grad_vs_oracle, _gpu_rollout
    case = TP.large_angle_grad_case()
    _, ret, ga, gd, _ = _gpu_rollout(torch, case, _pa_bodies(pa, case["make"]()))
    _check_grad_vs_oracle(case, ret, ga, gd)
    assert np.nanmax(np.abs(gd[:, 4, :])) > 1e-3
