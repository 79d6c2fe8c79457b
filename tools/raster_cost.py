"""What pixel observations cost (perf tooling): 4096
envs on one MI355X, RoboCup (perturbed reset state) and LunarLander (a
terrain per env), 64 x 64 and 84 x 84, ids and planar RGB, the default window
and an egocentric camera, cotix_rasterize's two decompositions -- the
workgroup's four waves per env and one wave per env
(COTIX_RASTER_WAVE_PER_ENV) -- in alternation: device events around every
launch after warm-up, median (min - max) ms, and the written bytes over the
time against the 8 TB/s of HBM (a kernel far below it is compute-bound).
  python tools/raster_cost.py [--B 4096] [--reps 50] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
FORMS = {"workgroup_per_env": "0", "wave_per_env": "1"}


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def scenario(pa, name, B):
    dev = "cuda:0"
    if name == "robocup":
        return pa.RoboCupEnv(batch=B, device=dev, perturb=True), 4
    keys = pa.random.split(pa.random.PRNGKey(0, dev), B)
    return pa.LunarLander(key=keys, batch=B, device=dev), 0


def measure(pa, name, B, sizes, reps, warmup):
    scen, follow = scenario(pa, name, B)
    w = scen.world
    cams = {"default": pa.Camera(),
            "egocentric": pa.Camera(half_extent=(1.0, 0.75), follow_body=follow, follow_angle=True)}
    rows = []
    for side in sizes:
        for cam_name, cam in cams.items():
            for rgb in (False, True):
                out = torch.empty((B, 3, side, side) if rgb else (B, side, side), dtype=torch.uint8, device=w.device)
                pal = scen.palette if rgb else None

                def launch():
                    pa.render.pixels(w, side, side, cam, pal, out=out)

                ms, images = {k: [] for k in FORMS}, {}
                for r in range(warmup + reps):  # the two forms in alternation
                    for form, flag in FORMS.items():
                        os.environ["COTIX_RASTER_WAVE_PER_ENV"] = flag
                        torch.cuda.synchronize()
                        t = timed(launch)
                        if r >= warmup:
                            ms[form].append(t)
                        elif r == 0:
                            images[form] = out.clone()
                os.environ.pop("COTIX_RASTER_WAVE_PER_ENV", None)
                assert torch.equal(images["workgroup_per_env"], images["wave_per_env"])  # the same bits
                row = {"scene": name, "B": B, "width": side, "height": side, "camera": cam_name,
                       "channels": 3 if rgb else 1, "bytes_written": out.numel(), "reps": reps,
                       "nonzero_byte_fraction": float((images["wave_per_env"] != 0).float().mean().item())}
                for form, v in ms.items():
                    med = statistics.median(v)
                    row[form + "_ms"] = {"median": med, "min": min(v), "max": max(v)}
                    row[form + "_share_of_hbm_write_rate"] = out.numel() / (med * 1e-3) / HBM_BYTES_PER_S
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", default="robocup,lunar")
    ap.add_argument("--sizes", default="64,84")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import parallax_amd as pa
    if not torch.cuda.is_available():
        raise SystemExit("raster_cost.py needs a GPU")
    res = {"build": pa._ffi.lib.cotix_version().decode(), "device": torch.cuda.get_device_name(0),
           "method": "device events around each launch, %d warm-up rounds, %d alternated repetitions"
                     % (a.warmup, a.reps), "rows": []}
    for name in a.scenes.split(","):
        res["rows"] += measure(pa, name, a.B, [int(s) for s in a.sizes.split(",")], a.reps, a.warmup)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
