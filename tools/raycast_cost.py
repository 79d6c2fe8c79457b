"""What range-sensor observations cost (perf tooling):
4096 envs on one MI355X, RoboCup (perturbed reset state, the sensor on the
ball) and LunarLander (a terrain per env, the sensor on the lander), 32 and
128 rays, with and without follow_angle: device events around every launch
after warm-up, median (min - max) ms.  For scale, measured in the same run on
the same worlds: one cotix_observe launch and one cotix_rasterize 64 x 64 ids
launch.
  python tools/raycast_cost.py [--B 4096] [--reps 50] [--out FILE.json]"""
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


def stats(f, reps, warmup):
    for _ in range(warmup):
        timed(f)
    v = [timed(f) for _ in range(reps)]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def scenario(pa, name, B):
    dev = "cuda:0"
    if name == "robocup":
        return pa.RoboCupEnv(batch=B, device=dev, perturb=True), 4
    keys = pa.random.split(pa.random.PRNGKey(0, dev), B)
    return pa.LunarLander(key=keys, batch=B, device=dev), 0


def measure(pa, name, B, ray_counts, reps, warmup):
    scen, body = scenario(pa, name, B)
    w = scen.world
    rows = []
    for R in ray_counts:
        dirs = pa.RaySensor.fan(R).to(w.device)
        dist = torch.empty(B, R, dtype=torch.float32, device=w.device)
        hit = torch.empty(B, R, dtype=torch.uint8, device=w.device)
        for follow in (False, True):
            sensor = pa.RaySensor(body=body, follow_angle=follow, max_range=6.0)
            row = {"scene": name, "B": B, "n_rays": R, "follow_angle": follow, "reps": reps, "what": "cotix_raycast",
                   "ms": stats(lambda: pa.render.rays(w, sensor, dirs, out=dist, hit_out=hit), reps, warmup),
                   "hit_fraction": float((hit != 0).float().mean().item())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    obs = torch.empty(B, len(w.bodies), 6, dtype=torch.float32, device=w.device)
    image = torch.empty(B, 64, 64, dtype=torch.uint8, device=w.device)
    for what, f in (("cotix_observe", lambda: w.observe(out=obs)),
                    ("cotix_rasterize 64x64 ids", lambda: pa.render.pixels(w, 64, 64, out=image))):
        row = {"scene": name, "B": B, "reps": reps, "what": what, "ms": stats(f, reps, warmup)}
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
        raise SystemExit("raycast_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "device": torch.cuda.get_device_name(0),
           "method": "device events around each launch, %d warm-up launches, %d timed launches"
                     % (a.warmup, a.reps), "rows": []}
    for name in a.scenes.split(","):
        res["rows"] += measure(pa, name, a.B, [int(r) for r in a.rays.split(",")], a.reps, a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
