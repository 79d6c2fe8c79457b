"""Kernel resource usage of two source trees side by side (perf tooling): the
null-path check of a change that adds kernel instantiations.  Compiles
cotix_step_kernel.hip of both trees for every envs-per-wave tiling (device
only, -Rpass-analysis=kernel-resource-usage, in parallel) and compares VGPRs,
SGPRs, spills, scratch and static LDS of every kernel (by mangled name) that
exists in tree A; kernels only in B are listed.  Exit 1 on any difference.
  python tools/res_compare.py TREE_A TREE_B [OUT.json]"""
import json
import os
import re
import subprocess
import sys
import tempfile

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "LDS Size", "Occupancy")


def compile_jobs(tree, tmp):
    jobs = []
    for ew in (1, 2, 4, 8):
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-ffp-contract=off",
               "-fno-fast-math", "-std=c++17", "--cuda-device-only", "-c", "-DCOTIX_EW=%d" % ew,
               os.path.join(tree, "parallax_amd", "csrc", "cotix_step_kernel.hip"), "-o",
               os.path.join(tmp, "ew%d.o" % ew), "-Rpass-analysis=kernel-resource-usage"]
        jobs.append((ew, subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
    return jobs


def parse(jobs):
    rows = {}
    for ew, p in jobs:
        err = p.communicate()[1]
        if p.returncode != 0:
            raise RuntimeError(err[-2000:])
        cur = None
        for ln in err.split("\n"):
            m = re.search(r"Function Name: (\S+)", ln)
            if m:
                # (a trailing defaulted `false` / 0 template argument is the same kernel, and
                # the gradient level that was a bool is the same kernel at the same value)
                cur = re.sub(r"(step_kernelILi\d+ELi\d+ELi\d+ELi\d+E)L[bi]0E", r"\1", m.group(1))
                cur = "ew%d %s" % (ew, re.sub(r"(step_kernelILi\d+ELi\d+ELi\d+ELi\d+E)Lb1E", r"\1Li1E", cur))
                rows[cur] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
            if m and cur and m.group(1).strip() in FIELDS:
                rows[cur][m.group(1).strip()] = int(m.group(2))
    return rows


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ja, jb = compile_jobs(a_dir, ta), compile_jobs(b_dir, tb)
        a, b = parse(ja), parse(jb)
    diff = {k: (a[k], b.get(k)) for k in a if a[k] != b.get(k)}
    new = sorted(k for k in b if k not in a)
    print("%d kernels in A, %d in B; %d of A's differ; %d only in B" % (len(a), len(b), len(diff), len(new)))
    for k, (x, y) in diff.items():
        print("DIFF", k, x, y)
    for k in new:
        v = b[k]
        print("NEW ", k, " ".join("%s=%s" % (f, v.get(f)) for f in FIELDS))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump({"a": a, "b": b, "differ": sorted(diff), "only_in_b": new}, f, indent=1, sort_keys=True)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
