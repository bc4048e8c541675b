#!/usr/bin/env python3
"""Per-kernel register use and spills of the HIP translation units
(icp_kernels, rgbd_align, viewer_cloud, voxel_map, map_render, depth_filter, rectify, loop_close)
as hipcc reports them
(-Rpass-analysis=kernel-resource-usage): `python tools/kres.py [filter]`
compiles each TU for gfx950 with the product flags (object discarded) and
prints VGPRs / AGPRs / SGPRs / spills / LDS / occupancy per kernel
(`python tools/kres.py rgbd`: k_rgbd_prep and k_rgbd_reduce, profiles/rgbd/kres_rgbd.txt).
tools/kernel_reach.py takes its list of instantiations from here (compiled_kernels)."""
import re
import subprocess
import sys

ROOT = __file__.rsplit("/tools/", 1)[0]
UNITS = ("icp_kernels", "rgbd_align", "viewer_cloud", "voxel_map", "map_render", "depth_filter",
         "rectify", "loop_close")


def kernel_name(demangled):
    """A demangled kernel symbol, with or without its return type, namespace and
    argument list -> `k_name` or `k_name<args>`, as every listing prints it."""
    s = re.sub(r"\(anonymous namespace\)::", "", demangled.strip())
    s = s.split("(")[0].strip()
    if s.endswith(" [clone .kd]"):
        s = s[:-len(" [clone .kd]")]
    return re.sub(r"^void\s+", "", s)


def compiled_kernels(units=UNITS):
    """{kernel_name: {"unit": translation unit, remark: value, ...}} of every
    kernel hipcc emits for the units, in the compiler's order."""
    rows = {}
    for tu in units:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
               "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", f"-I{ROOT}/include",
               f"-I{ROOT}/slam-rgbd_amd/csrc", "-c", f"{ROOT}/slam-rgbd_amd/csrc/{tu}.hip",
               "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
        out = subprocess.run(cmd, capture_output=True, text=True).stderr
        cur = None
        for ln in out.splitlines():
            m = re.search(r"remark: ([A-Za-z ]+?)(?: \[[^\]]*\])?: (.+?)\s*\[-Rpass", ln)
            if not m:
                continue
            k, v = m.group(1).strip(), m.group(2).strip()
            if k == "Function Name":
                cur = kernel_name(subprocess.run(["c++filt", v], capture_output=True, text=True).stdout)
                rows[cur] = {"unit": tu}
            elif cur:
                rows[cur][k] = v
    return rows


def main():
    flt = sys.argv[1] if len(sys.argv) > 1 else ""
    for name, r in compiled_kernels().items():
        if flt in name:
            print(f"{name:45s} VGPR {r.get('VGPRs','?'):>4s} AGPR {r.get('AGPRs','?'):>3s} "
                  f"SGPR {r.get('SGPRs','?'):>4s} spillV {r.get('VGPRs Spill','?'):>4s} "
                  f"spillS {r.get('SGPRs Spill','?'):>4s} scratch {r.get('ScratchSize','?'):>4s} "
                  f"LDS {r.get('LDS Size','?'):>6s} "
                  f"occ {r.get('Occupancy','?')}")


if __name__ == "__main__":
    main()
