"""Build the native library in-tree: hipcc --offload-arch=gfx950 -> cpprcoder_amd/librcx.so.

hipcc cross-compiles gfx950 without a GPU, so this also runs in the CPU-only build container.
"""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librcx.so")
LIB_VARIANTS = os.path.join(HERE, "librcx_variants.so")  # diagnostic: + the superseded kernels of csrc/variants/ (RCX_LIBRARY=...)
SOURCES = ["rcx_api.hip", "rcx_comm.hip"]
HEADERS = ["rcx_lane.hpp", "rcx_geom.hpp", "rcx_buf.hpp", "rcx_ctx.hpp", "rcx_launch.hpp", "rcx_items.hpp", "rcx_host.hpp", "rcx_streams.hpp", "rcx_bwt_api.hpp", "rcx_divtab.hpp", "rcx_kernels.hpp", "rcx_adaptive.hpp", "rcx_quad.hpp", "rcx_mc.hpp", "rcx_static.hpp", "rcx_rans.hpp", "rcx_bwt.hpp", "rcx_bwt_tie.hpp", "rcx_crc.hpp", "rcx_crc_api.hpp", "rcx_stats.hpp", "rcx_stats_api.hpp", "rcx_stored.hpp", "rcx_stored_api.hpp", "rcx_stored_items.hpp", "rcx_stored_items_api.hpp", "rcx_planes.hpp", "rcx_predict.hpp", "rcx_typed_api.hpp", "rcx_typed_items.hpp", "rcx_typed_items_api.hpp", "rcx_base.hpp", "rcx_base_api.hpp", "rcx_base_items.hpp", "rcx_base_items_api.hpp", "rcx_typed_stats.hpp", "rcx_typed_stats_api.hpp", "rcx_picks.hpp", "rcx_picks_api.hpp", "rcx_class_plan.hpp", "rcx_typed_picks.hpp", "rcx_typed_picks_api.hpp", "rcx_base_picks.hpp", "rcx_base_picks_api.hpp", "rcx_encode_picks.hpp", "rcx_encode_picks_api.hpp", "rcx_typed_split_picks.hpp", "rcx_typed_split_picks_api.hpp", os.path.join("variants", "rcx_variants.hpp"), "rcx_comm.hip", os.path.join("..", "..", "include", "rcx.h"), os.path.join("..", "..", "include", "rcx_planes.h"), os.path.join("..", "..", "include", "rcx_predict.h"), os.path.join("..", "..", "include", "rcx_stats.h"), os.path.join("..", "..", "include", "rcx_stored.h"), os.path.join("..", "..", "include", "rcx_stored_items.h"), os.path.join("..", "..", "include", "rcx_typed_items.h"), os.path.join("..", "..", "include", "rcx_base.h"), os.path.join("..", "..", "include", "rcx_base_items.h"), os.path.join("..", "..", "include", "rcx_typed_stats.h"), os.path.join("..", "..", "include", "rcx_picks.h"), os.path.join("..", "..", "include", "rcx_typed_picks.h"), os.path.join("..", "..", "include", "rcx_base_picks.h"), os.path.join("..", "..", "include", "rcx_encode_picks.h"), os.path.join("..", "..", "include", "rcx_typed_split_picks.h")]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built")


def stale(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False, variants: bool = False) -> str:
    """librcx.so, the product; variants=True: librcx_variants.so, the same + the superseded kernels (csrc/variants/), which the
    product does not carry -- tests/test_gpu_parity.py checks them through it, tools compare against them."""
    lib = LIB_VARIANTS if variants else LIB
    if not force and not stale(lib):
        return lib
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value"] + (["-DRCX_WITH_VARIANTS"] if variants else []) + [
           "-o", lib] + [os.path.join(CSRC, s) for s in SOURCES] + ["-L/opt/rocm/lib", "-lrccl"]  # rcx_comm.hip: RCCL
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(" ".join(cmd))
        print(proc.stdout, proc.stderr)
    if proc.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + proc.stderr[-4000:])
    return lib


if __name__ == "__main__":
    import sys
    print(build(force=True, verbose=True, variants="--variants" in sys.argv))
