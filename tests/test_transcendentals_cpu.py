"""What sincos32 / atan2_32 compute, against float64 (numpy's sin / cos /
arctan2 of the input widened to float64, themselves cross-checked with mpmath).

The three copies of the kernels -- the Python oracle (cotix_oracle.geometry),
its C port (oracle/c/cotix_oracle.c) and the kernels' own code on the host
(parallax_amd/csrc/cotix_device.h through tests/emu) -- are each held to

    |sin - ref|, |cos - ref| <= 2^-23      for every finite float32
    |s^2 + c^2 - 1|          <= 2^-22
    atan2: <= 2 ulp of the float64 result rounded to float32

and to one another bit for bit, on tests/transcendental_probes.py: every
binade, the float32 nearest multiples of pi/2 (dense across the 8192 seam
between the three-constant reduction and the exact one), the arguments at
which a float-only reduction breaks down (6.6e6, 2^31 * pi/2) and FLT_MAX.

Maxima measured here: sin/cos 6.7e-8 up to 8192 and 7.1e-8 beyond,
|s^2 + c^2 - 1| 1.15e-7, atan2 1.46 ulp.  With the float-only reduction
alone the sin/cos test fails (errors of 0.03 from 1e5, unbounded from 6.6e6);
with cephes's two-interval atan the atan2 test fails (2.77 ulp on these
pairs: results in [0.39, 0.5) came from pi/4 minus a number of twice their
ulp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

import transcendental_probes as TP  # noqa: E402

F = np.float32


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def copies():
    """{name: (sincos(x) -> (s, c), atan2(y, x) -> a)} of the three copies;
    a missing checker is built, never skipped."""
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "build/libcotix_emu.so"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "..", "oracle")], check=True)
    import emu
    from cotix_oracle import cport
    from cotix_oracle import geometry as G
    el, cl = emu.load(), cport.load()
    p = lambda a: a.ctypes.data_as(emu.P_)  # noqa: E731

    def native(fs, fa):
        def sincos(x):
            x = np.ascontiguousarray(x, F)
            s, c = np.zeros_like(x), np.zeros_like(x)
            fs(p(x), x.size, p(s), p(c))
            return s, c

        def atan2(y, x):
            y, x = np.ascontiguousarray(y, F), np.ascontiguousarray(x, F)
            out = np.zeros_like(y)
            fa(p(y), p(x), y.size, p(out))
            return out
        return sincos, atan2

    def py_sincos(x):
        r = np.array([G.sincos32(v) for v in x], F).reshape(-1, 2)
        return r[:, 0].copy(), r[:, 1].copy()

    def py_atan2(y, x):
        return np.array([G.atan2_32(a, b) for a, b in zip(y, x)], F)

    return {"oracle": (py_sincos, py_atan2), "cport": native(cl.oracle_sincos, cl.oracle_atan2),
            "emu": native(el.emu_sincos, el.emu_atan2)}


@pytest.fixture(scope="module")
def results(copies):
    """Every copy's sin/cos of PROBES and atan2 of the pairs, computed once."""
    with np.errstate(all="ignore"):
        y, x = TP.atan2_pairs()
        return {k: (sc(TP.PROBES), at(y, x)) for k, (sc, at) in copies.items()}, (y, x)


def test_probe_set():
    """The probes are what the tests claim to cover."""
    x = TP.PROBES
    fin = x[np.isfinite(x)]
    assert 30000 < x.size < 80000
    e = np.frexp(np.abs(fin[fin != 0]).astype(np.float64))[1] - 1
    assert set(range(-126, 128)) <= set(e.tolist())
    assert (np.abs(fin) == TP.SEAM).any() and (np.abs(fin) == np.nextafter(TP.SEAM, F(np.inf))).any()
    assert ((np.abs(fin) > 6.5e6) & (np.abs(fin) < 6.7e6)).sum() > 2000
    assert (fin == TP.FLT_MAX).any() and np.isnan(x).any() and np.isinf(x).any()
    assert abs(float(TP.HALF_PI) - np.pi / 2) == 0.0
    # each listed multiple of pi/2 is within one float32 spacing of k * pi/2
    for k in (1, 5215, 5216, 20050, 1 << 31, round((1 << 100) / TP.HALF_PI), round((1 << 127) / TP.HALF_PI)):
        v = TP.nearest_f32(k)
        assert abs(TP.Fraction(float(v)) - k * TP.HALF_PI) <= TP.Fraction(float(np.spacing(v)))
        assert (x == v).any()


def test_reference_vs_mpmath():
    """numpy's float64 sin / cos / arctan2 (the reference of every bound
    below) against mpmath at 200 bits, on a few hundred probes of every size:
    within 2^-52, three millionths of the bounds they referee."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    fin = TP.PROBES[np.isfinite(TP.PROBES)]
    pick = fin[:: max(1, fin.size // 400)]
    big = fin[np.abs(fin) > 1e6]
    pick = np.concatenate([pick, big[:: max(1, big.size // 200)]]).astype(np.float64)
    worst = 0.0
    for v in pick:
        worst = max(worst, abs(float(mpmath.sin(mpmath.mpf(float(v))) - mpmath.mpf(float(np.sin(v))))),
                    abs(float(mpmath.cos(mpmath.mpf(float(v))) - mpmath.mpf(float(np.cos(v))))))
    assert worst <= 2.0 ** -52, worst
    y, x = TP.atan2_pairs(300, seed=6)
    for a, b in zip(y.astype(np.float64), x.astype(np.float64)):
        if a == 0:  # mpmath has no signed zero: IEEE's axis cases are asserted as such in test_atan2_accuracy
            continue
        ref = mpmath.atan2(mpmath.mpf(float(a)), mpmath.mpf(float(b)))
        got = float(np.arctan2(a, b))
        assert abs(float(ref - mpmath.mpf(got))) <= 2.0 ** -52 * max(abs(got), 2.0 ** -1022), (a, b)


def test_two_over_pi_table_vs_mpmath():
    """The oracle's 2/pi words are the first 224 bits of 2/pi; the C port's
    and the kernels' tables are held to it by the bit-for-bit test below."""
    mpmath = pytest.importorskip("mpmath")
    from cotix_oracle import geometry as G
    mpmath.mp.prec = 400
    z = int(mpmath.floor(2 / mpmath.pi * mpmath.mpf(2) ** 224))
    assert list(G.TWO_OVER_PI_WORDS) == [0] + [(z >> (32 * (6 - i))) & 0xFFFFFFFF for i in range(7)]
    # and, without mpmath's pi: 2/pi from the probes' integer pi
    assert abs(TP.Fraction(z, 1 << 224) * TP.HALF_PI - 1) < TP.Fraction(1, 1 << 220)


@pytest.mark.parametrize("copy", ["oracle", "cport", "emu"])
def test_sincos_accuracy(results, copy):
    """sin and cos of every finite float32 probe within 2^-23 of float64's,
    on the unit circle within 2^-22, signs right wherever the value is not
    within 1e-6 of zero; +-inf and NaN give (NaN, NaN)."""
    (s, c), _ = results[0][copy]
    x = TP.PROBES
    fin = np.isfinite(x)
    assert np.isnan(s[~fin]).all() and np.isnan(c[~fin]).all()
    xf = x[fin].astype(np.float64)
    sf, cf = s[fin].astype(np.float64), c[fin].astype(np.float64)
    rs, rc = np.sin(xf), np.cos(xf)
    with np.errstate(all="ignore"):
        es, ec, eu = np.abs(sf - rs), np.abs(cf - rc), np.abs(sf * sf + cf * cf - 1.0)
    es, ec, eu = (np.where(np.isnan(v), np.inf, v) for v in (es, ec, eu))
    small = np.abs(xf) <= float(TP.SEAM)
    print("%s: max |sin err| %.3g / %.3g, |cos err| %.3g / %.3g, |s2+c2-1| %.3g / %.3g (|x| <= 8192 / beyond)"
          % (copy, es[small].max(), es[~small].max(), ec[small].max(), ec[~small].max(), eu[small].max(),
             eu[~small].max()))
    k = int(np.argmax(np.maximum(es, ec)))
    assert max(es.max(), ec.max()) <= TP.SINCOS_TOL, (xf[k], sf[k], rs[k], cf[k], rc[k])
    assert eu.max() <= TP.UNIT_TOL, xf[int(np.argmax(eu))]
    for got, ref in ((sf, rs), (cf, rc)):
        m = np.abs(ref) > 1e-6
        assert np.array_equal(np.signbit(got[m]), np.signbit(ref[m]))
    # the quadrant: (s, c) lies in the reference's quadrant wherever that is unambiguous
    m = (np.abs(rs) > 1e-6) & (np.abs(rc) > 1e-6)
    assert np.array_equal((sf[m] > 0) * 2 + (cf[m] > 0), (rs[m] > 0) * 2 + (rc[m] > 0))


@pytest.mark.parametrize("copy", ["oracle", "cport", "emu"])
def test_atan2_accuracy(results, copy):
    """atan2_32 within 2 ulp of the float64 result rounded to float32 over
    exponents -149 .. 127 of both signs, ratios that underflow and whose
    inverse would overflow; signed zeros and axes exactly as numpy has them."""
    _, a = results[0][copy]
    y, x = results[1]
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    with np.errstate(all="ignore"):
        r32 = ref.astype(F)
    ulp = np.spacing(np.maximum(np.abs(r32), F(0))).astype(np.float64)
    err = np.abs(a.astype(np.float64) - ref) / ulp
    print("%s: atan2 max error %.3f ulp over %d pairs" % (copy, err.max(), err.size))
    k = int(np.argmax(err))
    assert err.max() <= 2.0, (y[k], x[k], a[k], ref[k])
    assert np.array_equal(np.signbit(a), np.signbit(r32))
    ax = (y == 0) | (x == 0)  # signed zeros and axes: numpy's values, bit for bit
    assert ax.sum() >= 16 and same_f32(a[ax], r32[ax])
    und = (r32 == 0) & (y != 0)  # a ratio below the subnormals: a zero of y's sign
    assert und.any() and np.array_equal(np.signbit(a[und]), np.signbit(y[und]))


def test_atan2_nan(copies):
    for name, (_, at) in copies.items():
        y = np.array([np.nan, 1.0, np.nan, np.nan, 0.0], F)
        x = np.array([1.0, np.nan, np.nan, 0.0, np.nan], F)
        assert np.isnan(at(y, x)).all(), name


def test_copies_agree_bit_for_bit(results, copies):
    """Python oracle == C port == the kernels' code on the host, on every
    probe (beyond 2^31 * pi/2 included, where the quadrant used to come from
    an out-of-range float -> int conversion) and a 200 x 200 atan2 grid."""
    r = results[0]
    for other in ("cport", "emu"):
        for k in (0, 1):
            assert same_f32(r["oracle"][0][k], r[other][0][k]), other
        assert same_f32(r["oracle"][1], r[other][1]), other
    yy, xx = TP.atan2_grid()
    assert yy.size == 200 * 200
    with np.errstate(all="ignore"):
        want = copies["oracle"][1](yy, xx)
        for other in ("cport", "emu"):
            assert same_f32(copies[other][1](yy, xx), want), other


def test_sincos_symmetry_and_seam(copies):
    """sin is odd and cos even, exactly, on both sides of the seam; at the
    seam itself (8192 takes the three-constant path, its successor the exact
    one) both paths are within the bound of each other's neighbour."""
    sc = copies["emu"][0]
    x = TP.PROBES[np.isfinite(TP.PROBES)]
    s, c = sc(x)
    sn, cn = sc(-x)
    assert same_f32(sn + F(0), -s + F(0)) and same_f32(cn, c)
    up = np.nextafter(TP.SEAM, F(np.inf))
    (s0, s1), (c0, c1) = sc(np.array([TP.SEAM, up], F))
    d = float(up) - float(TP.SEAM)
    assert abs(float(s1) - float(s0)) <= d + 2 * TP.SINCOS_TOL and abs(float(c1) - float(c0)) <= d + 2 * TP.SINCOS_TOL


# ---------------------------------------------------------------------------
# the paths the GPU tests (tests/test_gpu_transcendentals.py) read the
# kernels through, on the host emulation
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_cport(copies):
    import emu
    from cotix_oracle import cport
    return emu, emu.load(), cport, cport.load()


def _emu_prims(emu, lib, bodies, dyn):
    h, geom = emu.oracle_scene(lib, bodies)
    B = dyn.shape[2]
    n = lib.emu_render(h, dyn.ctypes.data_as(emu.P_), geom.ctypes.data_as(emu.P_), 0, B, None)
    prims = np.zeros((B, n, 4), F)
    assert lib.emu_render(h, dyn.ctypes.data_as(emu.P_), geom.ctypes.data_as(emu.P_), 0, B,
                          prims.ctypes.data_as(emu.P_)) == n
    return prims


def test_render_probe_returns_sincos_bits(emu_cport, results):
    """The GPU test reads sincos32 through cotix_render of the probe
    triangle: on the host that path returns sincos32's bits for every probe
    (up to the sign of a zero), so the device test may ask for the same."""
    emu, lib, _, _ = emu_cport
    x = np.ascontiguousarray(TP.PROBES)
    s, c = TP.sincos_from_triangle(_emu_prims(emu, lib, TP.probe_triangle_bodies(), TP.probe_dyn(x)))
    (ws, wc), _ = results[0]["emu"]
    assert same_f32(s + F(0), ws + F(0)) and same_f32(c + F(0), wc + F(0))


@pytest.mark.parametrize("nv", [3, 4, 6, 8])
def test_order_clockwise_vs_float64(emu_cport, nv):
    """order_clockwise (atan2_32 about the float32 mean, stable sort) of
    polygons of scale 2^-60 .. 2^60 about a far-off mean == the float64
    arctan2 order == the oracle's."""
    emu, lib, _, _ = emu_cport
    from cotix_oracle import geometry as G
    v, order = TP.clockwise_cases(nv)
    want = np.stack([p[o] for p, o in zip(v, order)])
    got = v.copy()
    lib.emu_order_clockwise(got.ctypes.data_as(emu.P_), got.shape[0], nv)
    assert same_f32(got, want)
    orc = np.array([G.order_clockwise([tuple(q) for q in p]) for p in v], F)
    assert same_f32(orc, want)


@pytest.mark.parametrize("EW", [1, 4, 8])
@pytest.mark.parametrize("scene", ["poly_box", "mixed_circle"])
def test_step_at_large_angles_vs_cport(emu_cport, scene, EW):
    """17 fused steps of bodies at angles 8191.9 .. 1e20 (some crossing the
    8192 seam both ways): the kernel logic == the C port bit for bit, trace
    included, and the rendered polygons keep their local edge lengths within
    4 * 2^-23 relative -- the rotation is orthonormal at every angle."""
    emu, lib, cport, cl = emu_cport
    bodies, dyn0, keys0, dynamic = TP.large_angle_case(scene)
    B, T, nb = dyn0.shape[2], 17, len(bodies)
    h, geom = emu.oracle_scene(lib, bodies)
    dyn, keys, err = dyn0.copy(), keys0.copy(), np.zeros(B, np.uint32)
    ch, cl_ = emu.step_ex(lib, h, dyn, keys, err, geom, 0, T, cport.STAGES_ROBOCUP, nb, E=EW)
    wd, wk, we = dyn0.copy(), keys0.copy(), np.zeros(B, np.uint32)
    wch, wcl = cport.Scene(cl, bodies).step_ex(wd, wk, we, T, cport.STAGES_ROBOCUP, trace=True, nthreads=1)
    assert same_f32(dyn, wd) and np.array_equal(keys, wk) and np.array_equal(err, we)
    assert np.array_equal(ch, wch) and np.array_equal(cl_, wcl)
    assert (wcl >= 0).any()
    a0, a1 = dyn0[dynamic, 4, :].astype(np.float64), wd[dynamic, 4, :].astype(np.float64)
    up = (np.abs(a0) < 8192) & (np.abs(a1) > 8192)
    down = (np.abs(a0) > 8192) & (np.abs(a1) <= 8192)
    assert up.sum() >= 2 and down.sum() >= 2, (up.sum(), down.sum())
    prims = _emu_prims(emu, lib, bodies, wd)
    worst = 0.0
    for i, part, off, n in TP.polygon_part_offsets(bodies):
        want = TP.local_edge_lengths(part)
        got = TP.rendered_edge_lengths(prims, off, n)
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    print("%s EW %d: max relative edge length error %.3g (bound %.3g)" % (scene, EW, worst, 4 * 2.0 ** -23))
    assert worst <= 4 * 2.0 ** -23


def test_rollout_grad_at_large_angles_vs_oracle(emu_cport):
    """The backward of a polygon scene whose bodies start at 3.0e4 and 1.0e7
    rad against the oracle's torch VJP chain (its _SinCos calls the same
    sincos32) at the case's own tolerance; returns bit for bit."""
    import grad_cases as GC
    emu, lib, _, _ = emu_cport
    case = TP.large_angle_grad_case()
    h, geom = emu.oracle_scene(lib, case["make"]())
    dyn = np.ascontiguousarray(case["S0"].transpose(1, 2, 0))
    keys = np.array(case["keys"], np.uint32, copy=True)
    err = np.zeros(dyn.shape[2], np.uint32)
    ret, sd, sk, tape = emu.rollout(lib, h, dyn, keys, err, geom, 0, 1 | 4 | 16, case["actions"], case["ab"],
                                    case["w"], E=4)
    ga, gd = emu.rollout_backward(lib, h, sd, sk, geom, 0, 1 | 4 | 16, case["actions"], case["ab"], case["w"], E=4,
                                  tape=tape)
    orc = GC.oracle(case)
    big = 0.0
    for e in orc:
        r, oga, ogS = orc[e]
        assert F(ret[e]).view(np.uint32) == F(r).view(np.uint32), (e, ret[e], r)
        ok, msg = GC.close(ga[:, e], oga, case["tol"], case["name"])
        assert ok, "env %d grad_action %s" % (e, msg)
        ok, msg = GC.close(gd[:, :, e], ogS, case["tol"], case["name"])
        assert ok, "env %d grad_dyn0 %s" % (e, msg)
        big = max(big, float(np.nanmax(np.abs(ogS[:, 4]))))
    assert big > 1e-3  # the angles' own gradients are in play
