"""What the shape geometry's gradient costs (perf tooling, DESIGN.md section
15): the rollout backward without a request, with grad_params, with grad_geom
and with both on the bench's three gradient workloads -- RoboCup 4096 x 64,
the box world 4096 x 64, LunarLander 4096 settled on the terrain x 64 -- one
forward each, then the backwards in alternation, device events around every
launch after warm-up.  Without a request RoboCup's tape backward is the split
producer / consumer form; with one the one-wave MODE 4 (COTIX_SPLIT_BWD=0 in
the environment gives the one-wave form without a request too).  On the
reference scenes it also times grad_params on the generic kernel: what their
specializations are worth on this chain (the level-2 kernels are generic).
--plain-only times the backward without a request alone: the figure to
compare between two library builds (COTIX_AMD_LIB), run in alternation.
  python tools/grad_geom_cost.py [--B 4096] [--T 64] [--reps 20] [--plain-only] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.grad_params_cost import workload  # noqa: E402


def measure(pa, name, B, T, reps, warmup, dev, plain_only):
    world, stages, ab = workload(pa, name, B, dev)
    gen = torch.Generator(device="cpu").manual_seed(1234)
    actions = (torch.randn(T, B, 2, generator=gen) * 0.1).to(dev)
    w = pa.rollout.ball_x_weights(len(world.bodies), ab)
    _, saved = pa.rollout_forward(world, actions, ab, w, stages=stages)
    runs = {"plain": lambda: pa.rollout_backward(world, saved)}
    if not plain_only:
        runs["with_grad_params"] = lambda: pa.rollout_backward(world, saved, want_params=True)
        runs["with_grad_geom"] = lambda: pa.rollout_backward(world, saved, want_geom=True)
        runs["with_both"] = lambda: pa.rollout_backward(world, saved, want_params=True, want_geom=True)
        if world.scene.variant()["specialization"] != "generic":
            # what a specialization is worth on this chain: the level-1 kernel
            # of the scene's specialization against the generic level-1 kernel
            # (the level-2 kernels are generic only)
            def generic_params():
                world.set_variant(0, False)
                try:
                    return pa.rollout_backward(world, saved, want_params=True)
                finally:
                    world.set_variant(0, True)
            runs["with_grad_params_generic"] = generic_params
    ms = {k: [] for k in runs}
    for _ in range(warmup):
        for f in runs.values():
            f()
    torch.cuda.synchronize()
    out = {}
    for _ in range(reps):  # alternating
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[k] = f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    row = {"B": B, "T": T, "reps": reps, "variant": world.scene.variant()}
    if not plain_only:
        gg = out["with_grad_geom"][2]
        row["geom_words"] = int(gg.shape[0])
        row["finite_geom_grad_env_fraction"] = float(torch.isfinite(gg).all(dim=0).float().mean().item())
        row["nonzero_geom_grad_env_fraction"] = float((torch.nan_to_num(gg, nan=1.0) != 0).any(dim=0).float().mean()
                                                      .item())
    for k, v in ms.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        if k != "plain":
            row[k + "_ratio_median"] = row[k + "_ms"]["median"] / row["plain_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="robocup,box,lunar")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import parallax_amd as pa
    if not torch.cuda.is_available():
        raise SystemExit("grad_geom_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "split_bwd_env": os.environ.get("COTIX_SPLIT_BWD"),
           "device": torch.cuda.get_device_name(0), "rows": {}}
    for name in a.scenes.split(","):
        res["rows"][name] = measure(pa, name, a.B, a.T, a.reps, a.warmup, "cuda:0", a.plain_only)
        print(json.dumps({name: res["rows"][name]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
