"""Build libvrt_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m voxel_rt2_amd.build [--force]

Flags that matter for the numeric contract (include/vrt_detmath.h): -ffp-contract=off so no
a*b+c is fused behind our back, no fast-math, correctly rounded f32 divide / sqrt (hipcc default,
stated explicitly), denormals kept.
"""
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libvrt_hip.so")
# the units that hold device code (tools/asm_diff.py, tools/kernel_resources.py), then the host side
KERNEL_SOURCES = ["vrt_kernels.hip", "vrt_scene_kernels.hip", "vrt_query_kernels.hip", "vrt_probe_kernels.hip", "vrt_sky_kernels.hip"]
SOURCES = KERNEL_SOURCES + ["vrt_api.hip"]
FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-fno-gpu-flush-denormals-to-zero",
    # no v_pk_{mul,add,fma}_f32: the two-lane forms need their operands in aligned register pairs, and the moves and the register
    # pressure that buys cost more than the halved issue count saves -- the render kernels spill 16-17 registers with them and
    # none without (same IEEE results per component; config 2 +6 %, sun-lit +6 %, config 3 +4 %, dense 4K +1.5 %).  The host
    # pass ignores the feature name with a warning.
    "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
    "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-value", "-Wno-unused-result",
]
LINK_FLAGS = ["--offload-arch=gfx950", "-fPIC", "-shared"]   # of FLAGS, what the link of the units' objects takes


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libvrt_hip.so cannot be built (there is no CPU fallback)")


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd), flush=True)
    return subprocess.run(cmd, capture_output=True, text=True)


def _deps():
    d = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    inc = os.path.join(os.path.dirname(HERE), "include")
    d += [os.path.join(inc, f) for f in os.listdir(inc)]
    d.append(os.path.abspath(__file__))
    return d


def is_stale():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(p) > t for p in _deps())


def source_id():
    """sha256 (first 16 hex digits) over the sources and flags the library is built from: vrt_build_id()."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(os.path.dirname(HERE), "include")
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))
    files += sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()[:16]


def build(force=False, verbose=False, extra_flags=(), out=None):
    """out: an A/B variant (build_variants/libvrt_<name>.so, loaded through VRT_LIB_PATH) instead of the shipped library."""
    if out is None and not force and not is_stale():
        return OUT
    out = out or OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tag = source_id() + ("+" + "".join(extra_flags) if extra_flags else "")
    # The units are compiled side by side, one hipcc process each (one command over all of them compiles them one after the other),
    # into objects in a folder that goes away, and linked once.
    compile_flags = [f for f in FLAGS if f != "-shared"] + list(extra_flags) + [f'-DVRT_BUILD_ID="{tag}"']
    with tempfile.TemporaryDirectory() as tmp:
        objs = [os.path.join(tmp, os.path.splitext(s)[0] + ".o") for s in SOURCES]
        cmds = [[_hipcc()] + compile_flags + ["-c", os.path.join(CSRC, s), "-o", o] for s, o in zip(SOURCES, objs)]
        with ThreadPoolExecutor(max_workers=len(cmds)) as pool:
            steps = list(pool.map(lambda c: _run(c, verbose), cmds))
        if all(r.returncode == 0 for r in steps):
            steps.append(_run([_hipcc()] + LINK_FLAGS + objs + ["-o", out], verbose))
    if any(r.returncode != 0 for r in steps):
        sys.stderr.write("".join(r.stdout + r.stderr for r in steps))
        raise RuntimeError("hipcc failed building libvrt_hip.so")
    if verbose:
        sys.stderr.write("".join(r.stderr for r in steps))
    return out


if __name__ == "__main__":
    # python -m voxel_rt2_amd.build [--force]                      the shipped library
    # python -m voxel_rt2_amd.build --variant NAME -DFLAG ...      build_variants/libvrt_NAME.so with extra flags (A/B runs)
    if "--variant" in sys.argv:
        i = sys.argv.index("--variant")
        name, extra = sys.argv[i + 1], [a for a in sys.argv[i + 2:] if a.startswith("-")]
        print(build(force=True, extra_flags=extra, out=os.path.join(os.path.dirname(HERE), "build_variants", f"libvrt_{name}.so")))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
