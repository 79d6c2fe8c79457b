"""What the differentiable eval costs (perf tooling):
4096 envs, RoboCup and the box world, 8 NFEs x 8 env-steps, device events
around every launch after warm-up, the compared launches in alternation:

  forward   cotix_eval, the saving cotix_eval_rollout, and cotix_rollout_ex at
            64 steps
  backward  cotix_eval_backward against cotix_rollout_backward_ex's one-wave
            tape form at 64 steps (COTIX_SPLIT_BWD=0, set here: the split form
            does not carry the control's gradient either)

Every forward restarts from the same state (a copy per launch, outside the
timed region).  --only-eval times env.eval alone with whichever build
COTIX_AMD_LIB names: run it once per build, the two builds in alternation, to
show that the unchanged cotix_eval did not move against the parent commit.
  python tools/eval_grad_cost.py [--B 4096] [--reps 20] [--only-eval] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

os.environ.setdefault("COTIX_SPLIT_BWD", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def judge_control(pa, name, ab):
    """The tests' device pairs: RoboCup's goal judge, the box world's piecewise rate with a saturating control."""
    import eval_device_cases as EDC
    j, c = EDC.judges("goal" if name == "robocup" else "piecewise", ab)
    return pa.LinearJudge(**j), pa.AffineControl(**c)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(pa, name, B, nfe, wfe, reps, warmup):
    from parallax_amd import envs as E
    dev = "cuda:0"
    scen = pa.BoxWorld(batch=B, device=dev) if name == "box" else pa.RoboCupEnv(batch=B, device=dev, perturb=True)
    w = scen.world
    nb, T, dt, stages = len(w.bodies), nfe * wfe, 1e-2, pa._ffi.STAGES_ROBOCUP
    ab = nb - 1
    judge, control = judge_control(pa, name, ab)
    js, cs = judge.c_struct(), control.c_struct()
    dyn0, keys0 = w.dyn.clone(), w.keys.clone()
    st = E.WorldState(w.dyn.clone(), w.keys.clone(), w.err.clone())
    reward = torch.zeros(B, device=dev)
    fin = torch.zeros(B, dtype=torch.int32, device=dev)
    ptr, sp = pa._ffi.ptr, pa._ffi.stream_ptr

    def reset():
        st.dyn.copy_(dyn0)
        st.keys.copy_(keys0)
        st.err.zero_()
        reward.zero_()
        fin.zero_()

    def eval_with(lib):
        return lambda: pa._ffi.check(lib.cotix_eval(
            w.scene.handle, ptr(st.dyn), ptr(st.keys), ptr(st.err), ptr(w.geom), w.geom_stride, B, nfe, wfe, dt, stages,
            js, cs, None, 0, ptr(reward), ptr(fin), 0, None, None, None, sp(dev)), "cotix_eval")

    env = E.AbstractEnvironment(E.PhysicsWorld(w, stages), st, control, judge)
    period = float(dt * T)
    _, _, saved = pa.eval_forward(env, period, nfe, wfe)
    actions = torch.zeros(T, B, 2, device=dev)
    rw = pa.rollout.ball_x_weights(nb, ab)

    _, rsaved = pa.rollout_forward(w, actions, ab, rw, dt=dt, stages=stages)
    fwd = {"cotix_eval": eval_with(pa._ffi.lib),
           "cotix_eval_rollout": lambda: pa.eval_forward(env, period, nfe, wfe),
           "cotix_rollout_ex": lambda: pa.rollout_forward(w, actions, ab, rw, dt=dt, stages=stages)}
    bwd = {"cotix_eval_backward": lambda: pa.eval_backward(saved),
           "cotix_rollout_backward_ex": lambda: pa.rollout_backward(w, rsaved, want_dyn0=True)}
    ms = {k: [] for k in list(fwd) + list(bwd)}
    for _ in range(warmup):
        for k, f in {**fwd, **bwd}.items():
            reset()
            f()
    torch.cuda.synchronize()
    for _ in range(reps):  # alternating
        for k, f in {**fwd, **bwd}.items():
            reset()
            if k == "cotix_rollout_ex":
                w.dyn.copy_(dyn0)
                w.keys.copy_(keys0)
                w.err.zero_()
            torch.cuda.synchronize()
            ms[k].append(timed(f))
    gc = pa.eval_backward(saved)[0]
    row = {"B": B, "n_nfe": nfe, "wfe": wfe, "reps": reps, "variant": w.scene.variant(),
           "done_env_fraction": float((saved["finished"] != 0).float().mean().item()),
           "finite_control_grad_env_fraction": float(torch.isfinite(gc).all(dim=0).float().mean().item())}
    for k, v in ms.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return row


def only_eval(pa, name, B, nfe, wfe, reps, warmup):
    """cotix_eval alone, of whichever library this process loaded (COTIX_AMD_LIB)."""
    from parallax_amd import envs as E
    dev = "cuda:0"
    scen = pa.BoxWorld(batch=B, device=dev) if name == "box" else pa.RoboCupEnv(batch=B, device=dev, perturb=True)
    w = scen.world
    judge, control = judge_control(pa, name, len(w.bodies) - 1)
    st = E.WorldState(w.dyn.clone(), w.keys.clone(), w.err.clone())
    env = E.AbstractEnvironment(E.PhysicsWorld(w, pa._ffi.STAGES_ROBOCUP), st, control, judge)
    period = float(1e-2 * nfe * wfe)
    ms = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t = timed(lambda: env.eval(period, nfe, wfe))
        if r >= warmup:
            ms.append(t)
    return {"B": B, "n_nfe": nfe, "wfe": wfe, "reps": reps,
            "env_eval_ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--nfe", type=int, default=8)
    ap.add_argument("--wfe", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="robocup,box")
    ap.add_argument("--only-eval", action="store_true",
                    help="time env.eval (cotix_eval plus its host side) alone: run once per build under COTIX_AMD_LIB, "
                         "alternating the two builds, for the parent / branch comparison of the unchanged program")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import parallax_amd as pa
    if not torch.cuda.is_available():
        raise SystemExit("eval_grad_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "lib": os.path.relpath(pa._ffi.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(0), "rows": {}}
    for name in a.scenes.split(","):
        if a.only_eval:
            res["rows"][name] = only_eval(pa, name, a.B, a.nfe, a.wfe, a.reps, a.warmup)
        else:
            res["rows"][name] = measure(pa, name, a.B, a.nfe, a.wfe, a.reps, a.warmup)
        print(json.dumps({name: res["rows"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
