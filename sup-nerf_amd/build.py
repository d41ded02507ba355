"""Build recipe for libsupnerf_hip.so (gfx950 only).  In-tree output so the .so travels with the repo
snapshot to the GPU box.  Used by __graft_entry__.build() and runnable by hand:

    python sup-nerf_amd/build.py [--force] [--verbose]
    python sup-nerf_amd/build.py --out PATH [-DNAME[=VALUE] ...] [EXTRA.hip ...]     (diagnostic builds: tools/build_*.sh)
"""
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsupnerf_hip.so")
STAMP = os.path.join(HERE, ".libsupnerf_hip.stamp")
SOURCES = ["snr_aux.hip", "snr_loss.hip", "snr_loop.hip", "snr_wgrad.hip", "snr_mlp.hip", "snr_mlp16.hip", "snr_mlp16_bwd.hip", "snr_mlp_bwd.hip", "snr_bf16.hip", "snr_decoder.hip", "snr_iso.hip", "snr_band.hip", "snr_iso_grad.hip", "snr_ray.hip", "snr_mesh.hip", "snr_simplify.hip", "snr_nearest.hip", "snr_inside.hip", "snr_raycast.hip", "snr_smooth.hip", "snr_raster.hip", "snr_paint.hip", "snr_scene_bwd.hip", "snr_scene_rows.hip", "snr_views.hip", "snr_cross.hip"]
HEADERS = ["snr_layout.h", "snr_device.hpp", "snr_host.hpp", "snr_mlp_core.hpp", "snr_mlp16_core.hpp", "snr_grid.hpp", "snr_packed_mesh.hpp", "snr_nearest_grid.hpp", "snr_scene_merge.hpp", os.path.join("..", "..", "include", "supnerf_hip.h")]
EXPORTS = "exports.map"        # linker version script: the library exports the C ABI (snr_*) and no other symbol
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def _digest():
    h = hashlib.sha256()
    for f in SOURCES + HEADERS + [EXPORTS]:
        p = os.path.join(CSRC, f)
        if os.path.exists(p):
            h.update(f.encode()); h.update(open(p, "rb").read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def build_library(force=False, verbose=False, defines=(), extra_sources=(), out=LIB):
    """Compile every .hip source for gfx950 and link the shared library.  Returns its path.  A diagnostic build (extra -D macros
    such as SNR_STAMPS, extra sources, or another output path) is always rebuilt and leaves the product library alone."""
    product = not defines and not extra_sources and out == LIB
    dig = _digest()
    if product and not force and os.path.exists(LIB) and os.path.exists(STAMP) and open(STAMP).read().strip() == dig:
        return LIB
    srcs = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.abspath(s) for s in extra_sources]
    flags = FLAGS + ["-D" + d for d in defines]
    if extra_sources:
        flags.append("-I" + CSRC)          # (a source outside csrc/ includes the library's headers)
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        procs = []
        for i, s in enumerate(srcs):
            o = os.path.join(tmp, f"{i}_{os.path.basename(s)[:-4]}.o")
            objs.append(o)
            cmd = [HIPCC] + flags + ["-c", s, "-o", o]
            if verbose:
                cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
                print(" ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for cmd, p in procs:
            log, _ = p.communicate()
            if verbose or p.returncode != 0:
                print(log)
            if p.returncode != 0:
                raise RuntimeError("hipcc failed: " + " ".join(cmd))
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, EXPORTS), "-o", out] + objs
        subprocess.check_call(cmd)
    if product:
        with open(STAMP, "w") as f:
            f.write(dig)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else LIB
    print(build_library(force="--force" in args, verbose="--verbose" in args, defines=[a[2:] for a in args if a.startswith("-D")],
                        extra_sources=[a for a in args if a.endswith(".hip")], out=out))
