"""In-tree builds of the native extensions.

Built .so files live next to the sources (they travel with gpurun snapshots
and are git-ignored), so a GPU box needs no JIT cache.  Used by
__graft_entry__.build() and the Makefile.
"""

from __future__ import annotations

import os
import subprocess
import sysconfig

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
GFX_ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _python_includes() -> list:
    import pybind11

    return [
        f"-I{sysconfig.get_paths()['include']}",
        f"-I{pybind11.get_include()}",
    ]


def _needs_build(out: str, *inputs: str) -> bool:
    """True when out is missing or any input is newer than it."""
    if not os.path.exists(out):
        return True
    built = os.path.getmtime(out)
    return any(os.path.getmtime(src) > built for src in inputs)


def _run(cmd: list) -> None:
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(
            f"build failed: {' '.join(cmd)}\n--- stdout ---\n{proc.stdout}"
            f"\n--- stderr ---\n{proc.stderr}"
        )


def build_drmctl(force: bool = False) -> str:
    src = os.path.join(PKG_DIR, "drmctl.cpp")
    out = os.path.join(PKG_DIR, "_drmctl.so")
    if force or _needs_build(out, src):
        _run(
            ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out]
            + _python_includes()
        )
    return out


# headers shared by the probe and the sweeps
_HIP_HEADERS = [os.path.join(PKG_DIR, h)
                for h in ("hip_util.h", "probe_kernels.h",
                          "sweep_table.h", "sweep_table_ext.h",
                          "hbm_pattern.h", "hbm_march.h", "lds_march.h",
                          "valu_kernels.h", "valu_table.h",
                          "valu_trans_gfx950.inc")]


def build_healthprobe(force: bool = False) -> str:
    src = os.path.join(PKG_DIR, "health_probe.hip")
    out = os.path.join(PKG_DIR, "_healthprobe.so")
    if force or _needs_build(out, src, *_HIP_HEADERS):
        _run(
            [
                HIPCC,
                f"--offload-arch={GFX_ARCH}",
                "-O3",
                "-std=c++17",
                "-shared",
                "-fPIC",
                src,
                "-o",
                out,
            ]
            + _python_includes()
        )
    return out


_FASTSERVER_HEADERS = [os.path.join(PKG_DIR, h)
                       for h in ("nghttp2_abi.h", "pref_alloc.h")]


def build_fastserver(force: bool = False) -> str:
    src = os.path.join(PKG_DIR, "fastserver.cpp")
    out = os.path.join(PKG_DIR, "_fastserver.so")
    if force or _needs_build(out, src, *_FASTSERVER_HEADERS):
        _run(
            ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out,
             "-ldl", "-pthread"]
            + _python_includes()
        )
    return out


def build_h2tool(force: bool = False) -> str:
    src = os.path.join(PKG_DIR, "h2tool.cpp")
    out = os.path.join(PKG_DIR, "_h2tool.so")
    hdr = os.path.join(PKG_DIR, "nghttp2_abi.h")
    if force or _needs_build(out, src, hdr):
        _run(
            ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out,
             "-ldl"]
            + _python_includes()
        )
    return out


def build_sweeps(force: bool = False) -> list:
    """The stand-alone mfma_bench / hbm_bench binaries that measure the
    probe's kernels against their variants; not part of build_all."""
    outs = []
    for name in ("mfma_bench", "hbm_bench"):
        out = os.path.join(PKG_DIR, name)
        src = out + ".hip"
        if force or _needs_build(out, src, *_HIP_HEADERS):
            _run([HIPCC, f"--offload-arch={GFX_ARCH}", "-O3", "-std=c++17",
                  src, "-o", out])
        outs.append(out)
    return outs


def build_all(force: bool = False) -> list:
    return [build_drmctl(force), build_healthprobe(force),
            build_fastserver(force), build_h2tool(force)]


if __name__ == "__main__":
    import sys

    force = "--force" in sys.argv
    build = build_sweeps if "--sweeps" in sys.argv else build_all
    for built in build(force):
        print(built)
