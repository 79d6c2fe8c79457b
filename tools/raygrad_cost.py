"""What range-sensor gradients cost (perf tooling):
4096 envs on one MI355X, RoboCup (perturbed reset state, the sensor on the
ball) and LunarLander (a terrain per env, the sensor on the lander, with
follow_angle), 32 and 128 rays.  cotix_raycast, cotix_raycast_backward with
g_dyn alone and with g_dyn and g_geom are alternated launch by launch: 3 warm-up
rounds, then `reps` timed rounds with device events around each launch; median
(min - max) ms, and the backward as a multiple of the forward of the same run.
  python tools/raygrad_cost.py [--B 4096] [--reps 50] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternated(fs, reps, warmup):
    """{name: ms stats} of the launches in `fs`, taken in turn."""
    for _ in range(warmup):
        for f in fs.values():
            timed(f)
    v = {k: [] for k in fs}
    for _ in range(reps):
        for k, f in fs.items():
            v[k].append(timed(f))
    return {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in v.items()}


def scenario(pa, name, B):
    dev = "cuda:0"
    if name == "robocup":
        return pa.RoboCupEnv(batch=B, device=dev, perturb=True), 4, False
    keys = pa.random.split(pa.random.PRNGKey(0, dev), B)
    return pa.LunarLander(key=keys, batch=B, device=dev), 0, True


def measure(pa, name, B, ray_counts, reps, warmup):
    scen, body, follow = scenario(pa, name, B)
    w = scen.world
    rows = []
    for R in ray_counts:
        dirs = pa.RaySensor.fan(R).to(w.device)
        dist = torch.empty(B, R, dtype=torch.float32, device=w.device)
        hit = torch.empty(B, R, dtype=torch.uint8, device=w.device)
        g = torch.rand(B, R, device=w.device) * 2.0 - 1.0
        sensor = pa.RaySensor(body=body, follow_angle=follow, max_range=6.0)
        ms = alternated({
            "cotix_raycast": lambda: pa.render.rays(w, sensor, dirs, out=dist, hit_out=hit),
            "cotix_raycast_backward g_dyn": lambda: pa.render.rays_backward(w, sensor, dirs, g),
            "cotix_raycast_backward g_dyn + g_geom":
                lambda: pa.render.rays_backward(w, sensor, dirs, g, want_geom=True),
        }, reps, warmup)
        fwd = ms["cotix_raycast"]["median"]
        for what, m in ms.items():
            row = {"scene": name, "B": B, "n_rays": R, "follow_angle": follow, "reps": reps, "what": what, "ms": m,
                   "times_forward": m["median"] / fwd, "geom_words": w.scene.geom_part_words,
                   "hit_fraction": float((hit != 0).float().mean().item())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="robocup,lunar")
    ap.add_argument("--rays", default="32,128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import parallax_amd as pa
    if not torch.cuda.is_available():
        raise SystemExit("raygrad_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "device": torch.cuda.get_device_name(0),
           "method": "forward and backward launches alternated, device events around each launch, %d warm-up "
                     "rounds, %d timed rounds; the backward's outputs are allocated inside the timed span"
                     % (a.warmup, a.reps), "rows": []}
    for name in a.scenes.split(","):
        res["rows"] += measure(pa, name, a.B, [int(r) for r in a.rays.split(",")], a.reps, a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
