"""Native extension loaders.

On a GPU machine the HIP probe must NOT silently fall back: if CUDA/HIP
devices are visible but the extension is missing, loading raises so a broken
deployment is caught loudly (the plugin's compute path is the .so, not an
eager fallback).
"""

from __future__ import annotations

import importlib
import os
from typing import Optional

_DIR = os.path.dirname(os.path.abspath(__file__))


class NativeExtensionMissing(ImportError):
    pass


def _load(name: str):
    try:
        return importlib.import_module(f"{__name__}.{name}")
    except ImportError as e:
        raise NativeExtensionMissing(
            f"{name}.so not built under {_DIR}; run "
            f"python -m k8s_device_plugin_amd.native.build (error: {e})"
        ) from e


def load_drmctl(required: bool = False):
    """Raw-ioctl shim; optional — sysfs fallbacks cover a missing shim."""
    try:
        return _load("_drmctl")
    except NativeExtensionMissing:
        if required:
            raise
        return None


def _gpu_visible() -> bool:
    # cheap check without importing torch: any KFD GPU node present
    try:
        from ..topology import simple_health_check

        return os.path.exists("/dev/kfd") and simple_health_check()
    except Exception:
        return False


def load_healthprobe(required: Optional[bool] = None):
    """gfx950 deep probe; REQUIRED whenever a GPU is actually present."""
    if required is None:
        required = _gpu_visible()
    try:
        return _load("_healthprobe")
    except NativeExtensionMissing:
        if required:
            raise
        return None


def load_fastserver(required: bool = False):
    """Native DevicePlugin gRPC server (nghttp2 over UDS)."""
    try:
        return _load("_fastserver")
    except NativeExtensionMissing:
        if required:
            raise
        return None


# Performance floors for the deep probe.  Calibrated against our own
# MI355X measurements across BOTH conditions the probe runs in:
# standalone (1935-2043 TF/s bf16 MFMA, 5.1-6.3 TB/s HBM copy across
# boxes — profiles/r01_bench_mi355x.md, r01_pmc_mfma_peak.csv) and
# IN-BAND on a loaded daemon, where host-side churn and package-power
# shifting cost ~25-30% (worst healthy in-band observation: 1383 TF/s,
# r02 soak — an earlier 1450 floor false-positived there).  Floors sit
# ~25% under the worst healthy in-band number: they catch a halved
# matrix pipe or a downtrained HBM channel, never
# DVFS noise.  Overridable per deployment via env; 0 disables.
DEFAULT_MFMA_FLOOR_TFLOPS = 1000.0
DEFAULT_HBM_FLOOR_GBPS = 3800.0
MFMA_FLOOR_ENV = "AMDXDP_MFMA_FLOOR_TFLOPS"
HBM_FLOOR_ENV = "AMDXDP_HBM_FLOOR_GBPS"


def _floor_from_env(env: str, default: float) -> float:
    try:
        return float(os.environ[env])
    except (KeyError, ValueError):
        return default


CU_SWEEP_ENV = "AMDXDP_CU_SWEEP"
CU_SWEEP_INJECT_ENV = "AMDXDP_CU_SWEEP_INJECT"


def cu_sweep_enabled(cu_sweep: Optional[bool] = None) -> bool:
    """An explicit argument wins; None reads AMDXDP_CU_SWEEP (unset, empty
    or 0 = off)."""
    if cu_sweep is not None:
        return bool(cu_sweep)
    return os.environ.get(CU_SWEEP_ENV, "0").strip() not in ("", "0")


CU_SWEEP_EXTRA_ENV = "AMDXDP_CU_SWEEP_EXTRA"
# The pipes of each set, in the order of native/sweep_table.h and
# native/sweep_table_ext.h: an injection by name finds its set and index here.
CU_SWEEP_PIPES = {
    "base": ("bf16_16", "bf16_32", "f16_16", "fp8_16", "i8_16", "mxfp8_16"),
    "mx": ("mxfp4_16", "mxfp4_32", "mxfp6_16", "mxbf6_16", "mxfp8xfp4_16"),
    "wide": ("bf8_16", "f16_32", "fp8_32", "i8_32", "f64_16", "f32_16"),
}
CU_SWEEP_EXTRA_SETS = ("mx", "wide")


def cu_sweep_extra_sets(cu_sweep_extra=None) -> tuple:
    """The extra pipe sets to sweep, in the order mx, wide.  An explicit
    argument wins: "all", a comma list or an iterable of set names; None
    reads AMDXDP_CU_SWEEP_EXTRA (unset or empty = none)."""
    spec = cu_sweep_extra
    if spec is None:
        spec = os.environ.get(CU_SWEEP_EXTRA_ENV, "")
    if isinstance(spec, str):
        spec = [s.strip() for s in spec.split(",") if s.strip()]
    names = [str(s).strip().lower() for s in spec]
    if "all" in names:
        if len(names) != 1:
            raise ValueError("cu_sweep_extra: all stands alone")
        return CU_SWEEP_EXTRA_SETS
    for name in names:
        if name not in CU_SWEEP_EXTRA_SETS:
            raise ValueError(
                f"cu_sweep_extra: unknown pipe set {name!r}, expected all or "
                "some of " + ", ".join(CU_SWEEP_EXTRA_SETS))
    return tuple(s for s in CU_SWEEP_EXTRA_SETS if s in names)


def _sweep_inject_from_env(pipe_set: str = "base"):
    """AMDXDP_CU_SWEEP_INJECT="block:wave:pipe" -> (block, wave, pipe) for
    the set that owns the pipe, None for every other set: the sweep then
    simulates one bad matrix pipe on healthy hardware.  pipe is an index
    into the base set or the name of a pipe of any set."""
    spec = os.environ.get(CU_SWEEP_INJECT_ENV, "").strip()
    if not spec:
        return None
    fields = spec.split(":")
    try:
        block, wave = (int(x) for x in fields[:2])
        if len(fields) != 3:
            raise ValueError
        try:
            owner, pipe = "base", int(fields[2])
        except ValueError:
            name = fields[2].strip()
            owner = next(s for s, pipes in CU_SWEEP_PIPES.items()
                         if name in pipes)
            pipe = CU_SWEEP_PIPES[owner].index(name)
    except (ValueError, StopIteration):
        raise ValueError(
            f"{CU_SWEEP_INJECT_ENV}={spec!r}: expected block:wave:pipe, pipe "
            "an index into the base set or a pipe's name"
        ) from None
    return (block, wave, pipe) if owner == pipe_set else None


def cu_sweep_violations(sweep: dict) -> list:
    """One line per SIMD that failed the sweep."""
    return [
        "cu_sweep: xcc {xcc} se {se} cu {cu} simd {simd} failed {pipes}".format(
            xcc=b["xcc"], se=b["se"], cu=b["cu"], simd=b["simd"],
            pipes=",".join(b["pipes"]),
        )
        for b in sweep.get("bad", [])
    ]


def run_cu_sweep(device: int = 0, mod=None, pipe_set: str = "base") -> dict:
    """Known-answer MFMA sweep of every CU and SIMD of one HIP device, over
    the base pipes or one of the extra sets (CU_SWEEP_EXTRA_SETS)."""
    if mod is None:
        mod = load_healthprobe(required=True)
    inject = _sweep_inject_from_env(pipe_set)
    if pipe_set == "base":
        return mod.cu_sweep(device=device, inject=inject)
    return mod.cu_sweep(device=device, inject=inject, pipe_set=pipe_set)


def cu_sweep_incomplete_warning(sweep: dict, pipe_set: str = "base"):
    """The warning line of a sweep that found nothing bad but could not reach
    every SIMD, or None."""
    if not sweep.get("ok") or sweep.get("coverage_complete"):
        return None
    tag = "" if pipe_set == "base" else f"[{pipe_set}]"
    return "cu_sweep_incomplete{}: {} of {} CUs, {} SIMDs".format(
        tag, sweep.get("cus_covered"), sweep.get("cu_count"),
        sweep.get("simds_covered"))


VALU_SWEEP_ENV = "AMDXDP_VALU_SWEEP"
VALU_SWEEP_INJECT_ENV = "AMDXDP_VALU_SWEEP_INJECT"
# the op sets of native/valu_table.h, in its order
VALU_SWEEP_SETS = ("fma", "int", "cvt", "xlane", "salu", "trans")


def valu_sweep_sets(valu_sweep=None) -> tuple:
    """The VALU op sets to sweep, in the order of VALU_SWEEP_SETS.  An
    explicit argument wins: False or True (none, all), "all", a comma list or
    an iterable of set names; None reads AMDXDP_VALU_SWEEP (unset, empty or
    0 = none, 1 or all = every set, otherwise a comma list)."""
    spec = valu_sweep
    if spec is None:
        spec = os.environ.get(VALU_SWEEP_ENV, "")
    if spec is False:
        return ()
    if spec is True:
        return VALU_SWEEP_SETS
    if isinstance(spec, str):
        spec = [s.strip() for s in spec.split(",") if s.strip()]
    names = [str(s).strip().lower() for s in spec]
    if names in (["0"], []):
        return ()
    if "all" in names or "1" in names:
        if len(names) != 1:
            raise ValueError("valu_sweep: all stands alone")
        return VALU_SWEEP_SETS
    for name in names:
        if name not in VALU_SWEEP_SETS:
            raise ValueError(
                f"valu_sweep: unknown op set {name!r}, expected all or "
                "some of " + ", ".join(VALU_SWEEP_SETS))
    return tuple(s for s in VALU_SWEEP_SETS if s in names)


def _valu_op_names(mod, op_set: str) -> list:
    return [op["name"] for op in mod.valu_sweep_reference(op_set)["ops"]]


def _valu_inject_from_env(mod, op_set: str):
    """AMDXDP_VALU_SWEEP_INJECT="block:wave:op" -> (block, wave, index) for
    the set that owns the op, None for every other set: the sweep then
    simulates one bad op on healthy hardware.  op is the op's name."""
    spec = os.environ.get(VALU_SWEEP_INJECT_ENV, "").strip()
    if not spec:
        return None
    fields = spec.split(":")
    try:
        if len(fields) != 3:
            raise ValueError
        block, wave = (int(x) for x in fields[:2])
        name = fields[2].strip()
        owner = next(s for s in VALU_SWEEP_SETS
                     if name in _valu_op_names(mod, s))
    except (ValueError, StopIteration):
        raise ValueError(
            f"{VALU_SWEEP_INJECT_ENV}={spec!r}: expected block:wave:op, op "
            "the name of an op of one of the sets"
        ) from None
    if owner != op_set:
        return None
    return (block, wave, _valu_op_names(mod, owner).index(name))


def run_valu_sweep(device: int = 0, mod=None, op_set: str = "fma") -> dict:
    """Known-answer sweep of one VALU op set (VALU_SWEEP_SETS) over every CU
    and SIMD of one HIP device."""
    if mod is None:
        mod = load_healthprobe(required=True)
    inject = _valu_inject_from_env(mod, op_set)
    return mod.valu_sweep(device=device, inject=inject, op_set=op_set)


def valu_sweep_violations(sweep: dict, op_set: str = "") -> list:
    """One line per SIMD that failed the sweep of one set.  The scalar unit
    belongs to the CU: for set salu the SIMD is only where it was seen."""
    lines = []
    for b in sweep.get("bad", []):
        ops = ", ".join(b["ops"])
        if op_set == "salu":
            lines.append(
                "valu_sweep: xcc {} se {} cu {} scalar unit failed {} "
                "(seen by simd {})".format(b["xcc"], b["se"], b["cu"], ops,
                                           b["simd"]))
        else:
            lines.append("valu_sweep: xcc {} se {} cu {} simd {} failed {}".format(
                b["xcc"], b["se"], b["cu"], b["simd"], ops))
    return lines


def valu_sweep_incomplete_warning(sweep: dict, op_set: str):
    """The warning line of a set's sweep that found nothing bad but could
    not reach every SIMD, or None."""
    if not sweep.get("ok") or sweep.get("coverage_complete"):
        return None
    return "valu_sweep_incomplete[{}]: {} of {} CUs, {} SIMDs".format(
        op_set, sweep.get("cus_covered"), sweep.get("cu_count"),
        sweep.get("simds_covered"))


LDS_SWEEP_ENV = "AMDXDP_LDS_SWEEP"
LDS_SWEEP_INJECT_ENV = "AMDXDP_LDS_SWEEP_INJECT"


def lds_sweep_enabled(lds_sweep: Optional[bool] = None) -> bool:
    """An explicit argument wins; None reads AMDXDP_LDS_SWEEP (unset, empty
    or 0 = off)."""
    if lds_sweep is not None:
        return bool(lds_sweep)
    return os.environ.get(LDS_SWEEP_ENV, "0").strip() not in ("", "0")


def _lds_inject_from_env():
    """AMDXDP_LDS_SWEEP_INJECT="block:element:word:bit" -> the corruption
    that flips that bit of that block's LDS after step 0 of the first
    pattern of path b128: one bad LDS cell simulated on healthy hardware."""
    spec = os.environ.get(LDS_SWEEP_INJECT_ENV, "").strip()
    if not spec:
        return None
    try:
        block, element, word, bit = (int(x) for x in spec.split(":"))
    except ValueError:
        raise ValueError(
            f"{LDS_SWEEP_INJECT_ENV}={spec!r}: expected block:element:word:bit"
        ) from None
    return (block, "b128", "address", 0, "flip", element, word, bit)


def lds_sweep_violations(sweep: dict) -> list:
    """One line per CU whose LDS failed the sweep."""
    lines = []
    for b in sweep.get("bad", []):
        line = "lds_sweep: xcc {} se {} cu {}: {} bad accesses".format(
            b["xcc"], b["se"], b["cu"], b["mismatches"])
        first = b.get("first")
        if first:
            line += (" (path {} pattern {} step {}, element {}, bits {:#010x}"
                     " in word {})").format(
                first["path"], first["pattern"], first["step"],
                first["element"], first["got"] ^ first["expected"],
                first["word"])
        lines.append(line)
    return lines


def run_lds_sweep(device: int = 0, mod=None) -> dict:
    """March test of the whole LDS of every CU of one HIP device."""
    if mod is None:
        mod = load_healthprobe(required=True)
    return mod.lds_sweep(device=device, corrupt=_lds_inject_from_env())


HBM_SCRUB_ENV = "AMDXDP_HBM_SCRUB_BYTES"
HBM_SCRUB_DEFAULT_RESERVE = 2 << 30
# below this share of the card's VRAM a scrub of "all" says that it was partial
HBM_SCRUB_FULL_SHARE = 0.9


def hbm_scrub_bytes_from_env(hbm_scrub_bytes=None):
    """An explicit argument wins; None reads AMDXDP_HBM_SCRUB_BYTES.  Returns
    None (off: unset, empty or 0), "all" or a positive int."""
    spec = hbm_scrub_bytes
    if spec is None:
        spec = os.environ.get(HBM_SCRUB_ENV, "")
    if isinstance(spec, str):
        spec = spec.strip().lower()
        if spec in ("", "0"):
            return None
        if spec == "all":
            return "all"
        try:
            spec = int(spec, 0)
        except ValueError:
            raise ValueError(
                f"{HBM_SCRUB_ENV}={spec!r}: expected all or a byte count"
            ) from None
    spec = int(spec)
    if spec < 0:
        raise ValueError("hbm_scrub_bytes must not be negative")
    return spec or None


def read_ecc_counts(bdf: str, sysroot: str = "/", block: str = "umc"):
    """{"ue": n, "ce": n} from <sysroot>/sys/bus/pci/devices/<bdf>/ras/
    <block>_err_count (lines of `key: integer`, other keys ignored), or None
    when the file cannot be read or does not hold both.  block: "umc" is the
    HBM's counters, "gfx" those of the compute units, LDS included."""
    path = os.path.join(sysroot, "sys/bus/pci/devices", bdf, "ras",
                        f"{block}_err_count")
    counts = {}
    try:
        with open(path) as f:
            for line in f:
                key, sep, value = line.partition(":")
                if sep and key.strip() in ("ue", "ce"):
                    counts[key.strip()] = int(value.strip(), 0)
    except (OSError, ValueError):
        return None
    return counts if len(counts) == 2 else None


def hbm_scrub_violations(scrub: dict) -> list:
    """One line per bad 2 MiB-aligned range, one for an overwritten guard."""
    lines = []
    for r in scrub.get("bad_ranges", []):
        line = "hbm_scrub: {} bad elements in bytes {:#x}-{:#x}".format(
            r["mismatches"], r["start"], r["end"])
        first = r.get("first")
        if first:
            line += " (pattern {} step {}, bits {:#010x} in word {})".format(
                first["pattern"], first["step"],
                first["got"] ^ first["expected"], first["word"])
        lines.append(line)
    if scrub.get("guard_ok") is False:
        lines.append("hbm_scrub: guard band overwritten")
    return lines


def hbm_scrub(device: int = 0, bytes=None,
              reserve_bytes: int = HBM_SCRUB_DEFAULT_RESERVE,
              sysroot: str = "/", mod=None, patterns=None) -> dict:
    """In-place march test of device memory (native/hbm_march.h).

    bytes=None or "all" takes the free VRAM less reserve_bytes; run it on a
    drained node.  Adds `healthy`, `violations`, `warnings` and `ecc` (the
    umc_err_count counters before and after, None when unreadable) to the
    module's result.  A scrub of "all" that reached under 90 % of the card
    only warns: a scrub that could not look is not a sick GPU.
    """
    if mod is None:
        mod = load_healthprobe(required=True)
    whole = bytes is None or bytes == "all"
    if whole:
        free, _total = mod.mem_info(device)
        bytes = (int(free) - int(reserve_bytes)) // 16 * 16
        if bytes < 16:
            raise ValueError(
                f"hbm_scrub: {free} bytes free, reserve_bytes={reserve_bytes}"
                " leaves nothing to test")
    bdf = None
    try:
        bdf = mod.pci_bus_ids()[device].lower()
    except Exception:
        pass
    ecc_before = read_ecc_counts(bdf, sysroot) if bdf else None
    kwargs = {} if patterns is None else {"patterns": list(patterns)}
    res = mod.hbm_scrub(device=device, bytes=int(bytes), **kwargs)
    ecc_after = read_ecc_counts(bdf, sysroot) if bdf else None

    violations = hbm_scrub_violations(res)
    warnings = []
    if whole and res["bytes_tested"] < HBM_SCRUB_FULL_SHARE * res["vram_bytes"]:
        warnings.append("hbm_scrub_partial: tested {} of {} bytes".format(
            res["bytes_tested"], res["vram_bytes"]))
    res["ecc"] = None
    if ecc_before is not None and ecc_after is not None:
        res["ecc"] = {"before": ecc_before, "after": ecc_after}
        ue = ecc_after["ue"] - ecc_before["ue"]
        ce = ecc_after["ce"] - ecc_before["ce"]
        if ue > 0:
            violations.append(
                f"hbm_scrub: {ue} uncorrectable ECC errors during the scrub")
        if ce > 0:
            warnings.append(
                f"hbm_scrub_ecc: {ce} corrected ECC errors during the scrub")
    res["violations"] = violations
    res["warnings"] = warnings
    res["healthy"] = not violations
    return res


def lds_sweep_with_ecc(device: int = 0, mod=None, sysroot: str = "/") -> dict:
    """run_lds_sweep between two readings of the GPU's gfx RAS counters.

    Adds `violations`, `warnings` and `ecc` (gfx_err_count before and after,
    None when unreadable) to the module's result: LDS is ECC-protected, so a
    weak cell may show only as a corrected error.
    """
    if mod is None:
        mod = load_healthprobe(required=True)
    bdf = None
    try:
        bdf = mod.pci_bus_ids()[device].lower()
    except Exception:
        pass
    ecc_before = read_ecc_counts(bdf, sysroot, "gfx") if bdf else None
    res = run_lds_sweep(device, mod)
    ecc_after = read_ecc_counts(bdf, sysroot, "gfx") if bdf else None

    violations = lds_sweep_violations(res)
    warnings = []
    if res.get("ok") and not res.get("coverage_complete"):
        warnings.append("lds_sweep_incomplete: {} of {} CUs".format(
            res.get("cus_covered"), res.get("cu_count")))
    res["ecc"] = None
    if ecc_before is not None and ecc_after is not None:
        res["ecc"] = {"before": ecc_before, "after": ecc_after}
        ue = ecc_after["ue"] - ecc_before["ue"]
        ce = ecc_after["ce"] - ecc_before["ce"]
        if ue > 0:
            violations.append(
                f"lds_sweep: {ue} uncorrectable gfx ECC errors during the sweep")
        if ce > 0:
            warnings.append(
                f"lds_sweep_ecc: {ce} corrected gfx ECC errors during the sweep")
    res["violations"] = violations
    res["warnings"] = warnings
    return res


def deep_health_probe(
    device: int = 0,
    hbm_bytes: int = 1 << 30,
    mfma_floor_tflops: Optional[float] = None,
    hbm_floor_gbps: Optional[float] = None,
    cu_sweep: Optional[bool] = None,
    hbm_scrub_bytes=None,
    lds_sweep: Optional[bool] = None,
    sysroot: str = "/",
    cu_sweep_extra=None,
    valu_sweep=None,
) -> dict:
    """Run the on-GPU MFMA/LDS/HBM probe and apply performance floors.

    Raises loudly when the extension is missing on a GPU machine.  The
    result's `healthy` goes False on any correctness failure OR any floor
    violation; violations are listed in `floor_violations`.

    cu_sweep (None = env AMDXDP_CU_SWEEP, default off) adds the known-answer
    MFMA sweep of every CU and SIMD under `cu_sweep`: a bad SIMD makes the
    GPU unhealthy, with one violation line each; a sweep that could not reach
    every SIMD but found nothing bad only sets `warnings`.

    cu_sweep_extra (None = env AMDXDP_CU_SWEEP_EXTRA, default none; "all" or
    an iterable of "mx" / "wide") acts only while the CU sweep is on: the
    same sweep over the block-scaled fp4 / fp6 pipes (mx) and over bf8, the
    32x32 shapes, f64 and f32-input (wide), under `cu_sweep_extra` as
    {set: dict}, with the same violation lines and a warning of its own for a
    clean but incomplete set.

    hbm_scrub_bytes (None = env AMDXDP_HBM_SCRUB_BYTES, default off; "all" or
    a byte count) adds the march test of that much VRAM under `hbm_scrub`;
    its violations and warnings join `floor_violations` and `warnings`.

    lds_sweep (None = env AMDXDP_LDS_SWEEP, default off) adds the march test
    of every CU's whole LDS under `lds_sweep`: a CU with a bad access makes
    the GPU unhealthy, with one violation line each; a clean sweep that did
    not own every CU's LDS only warns.  The gfx RAS counters under sysroot
    are read before and after (`ecc`, None when unreadable): corrected
    errors during the sweep warn, uncorrectable ones are a violation.

    valu_sweep (None = env AMDXDP_VALU_SWEEP, default off; True, "all" or an
    iterable of VALU_SWEEP_SETS) adds the known-answer sweep of the vector,
    conversion, cross-lane, scalar and transcendental ops under `valu_sweep`
    as {set: dict}: a SIMD (set salu: a CU's scalar unit) with a wrong result
    makes the GPU unhealthy, with one violation line per SIMD and set; a
    clean but incomplete set only warns.
    """
    if mfma_floor_tflops is None:
        mfma_floor_tflops = _floor_from_env(MFMA_FLOOR_ENV,
                                            DEFAULT_MFMA_FLOOR_TFLOPS)
    if hbm_floor_gbps is None:
        hbm_floor_gbps = _floor_from_env(HBM_FLOOR_ENV,
                                         DEFAULT_HBM_FLOOR_GBPS)
    if cu_sweep_extra is not None:
        cu_sweep_extra = cu_sweep_extra_sets(cu_sweep_extra)  # or ValueError
    valu_sets = valu_sweep_sets(valu_sweep)  # or ValueError
    mod = load_healthprobe(required=True)
    res = mod.run_probe(device=device, hbm_bytes=hbm_bytes)
    violations = []
    if res.get("hbm_copy_ok") is False:
        # the whole copy is compared with the fill pattern on the device
        violations.append(
            "hbm_copy: {} elements differ from the pattern, first at {}".format(
                res.get("hbm_mismatches", "?"), res.get("hbm_first_bad", "?"))
        )
    mfma = res.get("mfma_tflops")
    if mfma_floor_tflops > 0 and mfma is not None and mfma < mfma_floor_tflops:
        violations.append(
            f"mfma_tflops {mfma:.0f} < floor {mfma_floor_tflops:.0f}"
        )
    hbm = res.get("hbm_gbps")
    if hbm_floor_gbps > 0 and hbm is not None and hbm < hbm_floor_gbps:
        violations.append(f"hbm_gbps {hbm:.0f} < floor {hbm_floor_gbps:.0f}")
    res["floors"] = {
        "mfma_tflops": mfma_floor_tflops,
        "hbm_gbps": hbm_floor_gbps,
    }
    if cu_sweep_enabled(cu_sweep):
        sweep = run_cu_sweep(device, mod)
        res["cu_sweep"] = sweep
        violations.extend(cu_sweep_violations(sweep))
        warning = cu_sweep_incomplete_warning(sweep)
        if warning:
            res["warnings"] = [warning]
        for pipe_set in cu_sweep_extra_sets(cu_sweep_extra):
            sweep = run_cu_sweep(device, mod, pipe_set)
            res.setdefault("cu_sweep_extra", {})[pipe_set] = sweep
            violations.extend(cu_sweep_violations(sweep))
            warning = cu_sweep_incomplete_warning(sweep, pipe_set)
            if warning:
                res.setdefault("warnings", []).append(warning)
    if lds_sweep_enabled(lds_sweep):
        sweep = lds_sweep_with_ecc(device, mod, sysroot)
        res["lds_sweep"] = sweep
        violations.extend(sweep["violations"])
        if sweep["warnings"]:
            res.setdefault("warnings", []).extend(sweep["warnings"])
    for op_set in valu_sets:
        sweep = run_valu_sweep(device, mod, op_set)
        res.setdefault("valu_sweep", {})[op_set] = sweep
        violations.extend(valu_sweep_violations(sweep, op_set))
        warning = valu_sweep_incomplete_warning(sweep, op_set)
        if warning:
            res.setdefault("warnings", []).append(warning)
    scrub_bytes = hbm_scrub_bytes_from_env(hbm_scrub_bytes)
    if scrub_bytes is not None:
        scrub = hbm_scrub(device, scrub_bytes, mod=mod)
        res["hbm_scrub"] = scrub
        violations.extend(scrub["violations"])
        if scrub["warnings"]:
            res.setdefault("warnings", []).extend(scrub["warnings"])
    res["floor_violations"] = violations
    if violations:
        res["healthy"] = False
    return res
