"""What the body parameters' gradient costs (perf tooling, DESIGN.md section
13): the rollout backward with and without grad_params on the bench's three
gradient workloads -- RoboCup 4096 x 64, the box world 4096 x 64, LunarLander
4096 settled on the terrain x 64 -- one forward each, then the two backwards
in alternation, device events around every launch after warm-up.  Without
grad_params RoboCup's tape backward is the split producer / consumer form;
with it the one-wave MODE 4 (COTIX_SPLIT_BWD=0 in the environment gives the
one-wave form without grad_params too, which separates the two costs).
  python tools/grad_params_cost.py [--B 4096] [--T 64] [--reps 20] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(pa, name, B, dev):
    stages, ab = pa._ffi.STAGES_ROBOCUP, None
    if name == "box":
        scen = pa.BoxWorld(batch=B, device=dev)
    elif name == "lunar":
        scen = pa.LunarLander(batch=B, device=dev)
        stages, ab = pa._ffi.STAGES_LUNAR | pa._ffi.STAGE_BROADPHASE, 0
        for _ in range(40):  # settled on the terrain (bench.py grad_lunar)
            scen.world.step(64, 1e-2, stages)
    else:
        scen = pa.RoboCupEnv(batch=B, device=dev, perturb=True)
    nb = len(scen.world.bodies)
    return scen.world, stages, nb - 1 if ab is None else ab


def measure(pa, name, B, T, reps, warmup, dev):
    world, stages, ab = workload(pa, name, B, dev)
    gen = torch.Generator(device="cpu").manual_seed(1234)
    actions = (torch.randn(T, B, 2, generator=gen) * 0.1).to(dev)
    w = pa.rollout.ball_x_weights(len(world.bodies), ab)
    _, saved = pa.rollout_forward(world, actions, ab, w, stages=stages)
    runs = {"plain": lambda: pa.rollout_backward(world, saved),
            "with_grad_params": lambda: pa.rollout_backward(world, saved, want_params=True)}
    ms = {k: [] for k in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    for _ in range(reps):  # alternating
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    gp = out[2]
    row = {"B": B, "T": T, "reps": reps, "variant": world.scene.variant(),
           "finite_param_grad_env_fraction": float(torch.isfinite(gp).all(dim=0).all(dim=0).float().mean().item())}
    for k, v in ms.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    row["ratio_median"] = row["with_grad_params_ms"]["median"] / row["plain_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="robocup,box,lunar")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import parallax_amd as pa
    if not torch.cuda.is_available():
        raise SystemExit("grad_params_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "split_bwd_env": os.environ.get("COTIX_SPLIT_BWD"),
           "device": torch.cuda.get_device_name(0), "rows": {}}
    for name in a.scenes.split(","):
        res["rows"][name] = measure(pa, name, a.B, a.T, a.reps, a.warmup, "cuda:0")
        print(json.dumps({name: res["rows"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
