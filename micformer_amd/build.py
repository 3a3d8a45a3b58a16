"""Build libmicformer_hip.so in-tree with hipcc for gfx950 (no torch involved: the library is a plain C-ABI .so)."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmicformer_hip.so")
SOURCES = ["linear.hip", "linear_grouped.hip", "head_tail.hip", "head_tail_fused.hip", "layernorm.hip", "window_attn.hip", "conv3.hip", "conv3_wgrad.hip", "conv3_direct.hip", "conv3_fwdx.hip", "conv3_bwdx.hip", "conv3_wgradx.hip", "offset_sample.hip", "patch.hip",
           "loss_optim.hip", "misc.hip", "block_fwd.hip", "block_bwd.hip", "block_wide.hip", "offset_head.hip", "grad_wire.hip",
           "surface_metrics.hip", "surface_distance.hip", "volume_loader.hip", "volume_normalise.hip", "volume_affine.hip", "volume_elastic.hip", "volume_intensity.hip", "volume_restore.hip", "volume_components.hip",
           "sliding_window.hip", "volume_patches.hip", "volume_patch_warp.hip", "volume_lowres.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fPIC", "-fvisibility=default"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libmicformer_hip.so)")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=True):
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_hip.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_metrics.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_surface.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_loader.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_normalise.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_affine.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_elastic.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_intensity.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_lowres.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_restore.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_components.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_blend.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_patches.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_patch_warp.h"))
    headers.append(os.path.join(os.path.dirname(HERE), "include", "micformer_mirror.h"))
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + headers):
            jobs.append((s, o))

    def compile_one(job):
        s, o = job
        cmd = [hipcc] + FLAGS + ["-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {s}:\n{r.stderr}")
        return s

    if jobs:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            for s in ex.map(compile_one, jobs):
                if verbose:
                    print(f"[micformer_amd.build] compiled {os.path.basename(s)}", file=sys.stderr)
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        if verbose:
            print(f"[micformer_amd.build] linked {LIB}", file=sys.stderr)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
