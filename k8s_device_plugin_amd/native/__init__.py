"""Native extension loaders.

On a GPU machine the HIP probe must NOT silently fall back: if CUDA/HIP
devices are visible but the extension is missing, loading raises so a broken
deployment is caught loudly (the plugin's compute path is the .so, not an
eager fallback).
"""

from __future__ import annotations

import importlib
import os
from dataclasses import dataclass
from typing import Callable, Optional

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
CU_SWEEP_EXTRA_ENV = "AMDXDP_CU_SWEEP_EXTRA"
# The pipes of each set, in the order of native/sweep_table.h and
# native/sweep_table_ext.h: an injection by name finds its set and index here.
CU_SWEEP_PIPES = {
    "base": ("bf16_16", "bf16_32", "f16_16", "fp8_16", "i8_16", "mxfp8_16"),
    "mx": ("mxfp4_16", "mxfp4_32", "mxfp6_16", "mxbf6_16", "mxfp8xfp4_16"),
    "wide": ("bf8_16", "f16_32", "fp8_32", "i8_32", "f64_16", "f32_16"),
}
CU_SWEEP_EXTRA_SETS = ("mx", "wide")

LDS_SWEEP_ENV = "AMDXDP_LDS_SWEEP"
LDS_SWEEP_INJECT_ENV = "AMDXDP_LDS_SWEEP_INJECT"

VALU_SWEEP_ENV = "AMDXDP_VALU_SWEEP"
VALU_SWEEP_INJECT_ENV = "AMDXDP_VALU_SWEEP_INJECT"
# the op sets of native/valu_table.h, in its order
VALU_SWEEP_SETS = ("fma", "int", "cvt", "xlane", "salu", "trans")

HBM_SCRUB_ENV = "AMDXDP_HBM_SCRUB_BYTES"
HBM_SCRUB_DEFAULT_RESERVE = 2 << 30
# below this share of the card's VRAM a scrub of "all" says that it was partial
HBM_SCRUB_FULL_SHARE = 0.9


# ---- what the opt-in checks share ----


def _switch_from_env(arg: Optional[bool], env: str) -> bool:
    """An explicit argument wins; None reads env (unset, empty or 0 = off)."""
    if arg is not None:
        return bool(arg)
    return os.environ.get(env, "0").strip() not in ("", "0")


def _sets_from(spec, env: str, what: str, noun: str, sets: tuple,
               switch: bool = False) -> tuple:
    """The sets that spec names, in the order of `sets`.  An explicit spec
    wins: "all", a comma list or an iterable of names; None reads env (unset
    or empty = none).  switch: False / True and "0" / "1" are none / all."""
    if spec is None:
        spec = os.environ.get(env, "")
    if switch and isinstance(spec, bool):
        return sets if spec else ()
    if isinstance(spec, str):
        spec = [s.strip() for s in spec.split(",") if s.strip()]
    names = [str(s).strip().lower() for s in spec]
    if switch and names == ["0"]:
        return ()
    if "all" in names or (switch and "1" in names):
        if len(names) != 1:
            raise ValueError(f"{what}: all stands alone")
        return sets
    for name in names:
        if name not in sets:
            raise ValueError(
                f"{what}: unknown {noun} {name!r}, expected all or "
                "some of " + ", ".join(sets))
    return tuple(s for s in sets if s in names)


def _inject_from_env(env: str, which: str, sets, names_of, expected: str,
                     index_set: Optional[str] = None):
    """env="block:wave:unit" -> (block, wave, index) for the set `which` if
    it owns the unit, None for every other set: the sweep then simulates one
    bad unit on healthy hardware.  unit is a name out of names_of(set) or,
    with index_set, an index into that set."""
    spec = os.environ.get(env, "").strip()
    if not spec:
        return None
    fields = spec.split(":")
    try:
        if len(fields) != 3:
            raise ValueError
        block, wave = (int(x) for x in fields[:2])
        unit = fields[2].strip()
        try:
            if index_set is None:
                raise ValueError
            owner, index = index_set, int(unit)
        except ValueError:
            owner = next(s for s in sets if unit in names_of(s))
            index = list(names_of(owner)).index(unit)
    except (ValueError, StopIteration):
        raise ValueError(f"{env}={spec!r}: expected {expected}") from None
    return (block, wave, index) if owner == which else None


def _simd_violations(key: str, sweep: dict, failed: str, sep: str,
                     scalar: bool = False) -> list:
    """One line per bad SIMD of a known-answer sweep.  scalar: the unit
    belongs to the CU, the SIMD is only where it was seen."""
    lines = []
    for b in sweep.get("bad", []):
        where = "{}: xcc {} se {} cu {}".format(key, b["xcc"], b["se"], b["cu"])
        names = sep.join(b[failed])
        if scalar:
            lines.append(f"{where} scalar unit failed {names} "
                         f"(seen by simd {b['simd']})")
        else:
            lines.append(f"{where} simd {b['simd']} failed {names}")
    return lines


def _incomplete_warning(key: str, sweep: dict, which: Optional[str] = None,
                        simds: bool = True):
    """The warning line of a sweep that found nothing bad but could not reach
    every CU (and SIMD), or None."""
    if not sweep.get("ok") or sweep.get("coverage_complete"):
        return None
    line = "{}_incomplete{}: {} of {} CUs".format(
        key, f"[{which}]" if which else "", sweep.get("cus_covered"),
        sweep.get("cu_count"))
    if simds:
        line += ", {} SIMDs".format(sweep.get("simds_covered"))
    return line


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


def _between_ecc_readings(sweep: "Sweep", run, device: int, mod, sysroot: str):
    """run() between two readings of the RAS counters that sweep.ecc names.
    Sets `ecc` on the result (before and after, None when unreadable) and
    returns (result, violations, warnings): uncorrectable errors during the
    run are a violation, corrected ones a warning."""
    block, label, act = sweep.ecc
    bdf = None
    try:
        bdf = mod.pci_bus_ids()[device].lower()
    except Exception:
        pass
    before = read_ecc_counts(bdf, sysroot, block) if bdf else None
    res = run()
    after = read_ecc_counts(bdf, sysroot, block) if bdf else None
    violations, warnings = [], []
    res["ecc"] = None
    if before is not None and after is not None:
        res["ecc"] = {"before": before, "after": after}
        ue = after["ue"] - before["ue"]
        ce = after["ce"] - before["ce"]
        if ue > 0:
            violations.append(f"{sweep.key}: {ue} uncorrectable {label}ECC "
                              f"errors during the {act}")
        if ce > 0:
            warnings.append(f"{sweep.key}_ecc: {ce} corrected {label}ECC "
                            f"errors during the {act}")
    return res, violations, warnings


@dataclass(frozen=True)
class Sweep:
    """One opt-in check of the deep probe.  `which` is one of the sets that
    select() returned: a set's name, or None for a sweep without sets and for
    the CU sweep's base set."""

    key: str                     # result key and prefix of its lines
    envs: tuple                  # the switch, then what chooses sets or injects
    select: Callable             # argument (None = env) -> the sets to run
    run: Callable = None         # (device, mod, which) -> result
    violations: Callable = None  # (result, which) -> lines
    incomplete: Callable = None  # (result, which) -> warning line or None
    sets: tuple = ()             # the set names select() accepts
    sets_key: str = None         # a named set's result goes here, {set: result}
    ecc: tuple = None            # RAS counters read before and after: (block,
    #                              its name in the lines, what ran)
    counts: str = None           # the plugin's bad-count gauge: distinct
    #                              "simds" over all sets, or "cus" summed
    # (result, which, ordinal) -> the plugin's own wording of the incomplete
    # line, where it does not log that line itself
    plugin_incomplete: Callable = None
    # (device, mod, which) -> (result, violations, warnings): a policy of its
    # own in place of check_sweep's
    check: Callable = None

    def place(self, res: dict, which, result: dict, ordinal=None) -> None:
        """Files a result under key, a named set's under sets_key as
        {set: result}; with an ordinal (the plugin) one level further down,
        as {ordinal: result}."""
        at, name = res, self.key
        if which is not None and self.sets_key:
            at, name = res.setdefault(self.sets_key, {}), which
        if ordinal is None:
            at[name] = result
        else:
            at.setdefault(name, {})[ordinal] = result


def check_sweep(sweep: Sweep, device: int = 0, which=None, mod=None,
                sysroot: str = "/"):
    """One run of a sweep on one HIP device -> (result, violation lines,
    warning lines).  A sweep with `ecc` runs between two readings of those
    RAS counters, and its result carries `ecc`, `violations` and `warnings`."""
    if mod is None:
        mod = load_healthprobe(required=True)
    if sweep.check:
        return sweep.check(device, mod, which)

    def run():
        return sweep.run(device, mod, which)
    res, ecc_violations, ecc_warnings = (
        _between_ecc_readings(sweep, run, device, mod, sysroot) if sweep.ecc
        else (run(), [], []))
    violations = sweep.violations(res, which) + ecc_violations
    warning = sweep.incomplete(res, which)
    warnings = ([warning] if warning else []) + ecc_warnings
    if sweep.ecc:
        res["violations"] = violations
        res["warnings"] = warnings
    return res, violations, warnings


# ---- CU sweep ----


def cu_sweep_enabled(cu_sweep: Optional[bool] = None) -> bool:
    """An explicit argument wins; None reads AMDXDP_CU_SWEEP (unset, empty
    or 0 = off)."""
    return _switch_from_env(cu_sweep, CU_SWEEP_ENV)


def cu_sweep_extra_sets(cu_sweep_extra=None) -> tuple:
    """The extra pipe sets to sweep, in the order mx, wide.  An explicit
    argument wins: "all", a comma list or an iterable of set names; None
    reads AMDXDP_CU_SWEEP_EXTRA (unset or empty = none)."""
    return _sets_from(cu_sweep_extra, CU_SWEEP_EXTRA_ENV, "cu_sweep_extra",
                      "pipe set", CU_SWEEP_EXTRA_SETS)


def _cu_sweep_select(arg) -> tuple:
    """(cu_sweep, cu_sweep_extra) -> None for the base set, then the extra
    sets; the extra sets act only while the sweep itself is on."""
    cu_sweep, extra = arg
    if not cu_sweep_enabled(cu_sweep):
        return ()
    return (None,) + cu_sweep_extra_sets(extra)


def run_cu_sweep(device: int = 0, mod=None, pipe_set: str = "base") -> dict:
    """Known-answer MFMA sweep of every CU and SIMD of one HIP device, over
    the base pipes or one of the extra sets (CU_SWEEP_EXTRA_SETS).
    AMDXDP_CU_SWEEP_INJECT="block:wave:pipe" simulates one bad matrix pipe:
    pipe is an index into the base set or the name of a pipe of any set."""
    if mod is None:
        mod = load_healthprobe(required=True)
    inject = _inject_from_env(
        CU_SWEEP_INJECT_ENV, pipe_set, CU_SWEEP_PIPES, CU_SWEEP_PIPES.get,
        "block:wave:pipe, pipe an index into the base set or a pipe's name",
        index_set="base")
    if pipe_set == "base":  # a module from before the extra sets has no such
        return mod.cu_sweep(device=device, inject=inject)  # parameter
    return mod.cu_sweep(device=device, inject=inject, pipe_set=pipe_set)


def cu_sweep_violations(sweep: dict) -> list:
    """One line per SIMD that failed the sweep."""
    return _simd_violations("cu_sweep", sweep, "pipes", ",")


def cu_sweep_incomplete_warning(sweep: dict, pipe_set: str = "base"):
    """The warning line of a sweep that found nothing bad but could not reach
    every SIMD, or None."""
    return _incomplete_warning("cu_sweep", sweep,
                               None if pipe_set == "base" else pipe_set)


CU_SWEEP = Sweep(
    key="cu_sweep",
    envs=(CU_SWEEP_ENV, CU_SWEEP_EXTRA_ENV, CU_SWEEP_INJECT_ENV),
    sets=CU_SWEEP_EXTRA_SETS, sets_key="cu_sweep_extra", counts="simds",
    select=_cu_sweep_select,
    run=lambda device, mod, which: run_cu_sweep(device, mod, which or "base"),
    violations=lambda sweep, which: cu_sweep_violations(sweep),
    incomplete=lambda sweep, which: cu_sweep_incomplete_warning(
        sweep, which or "base"),
    plugin_incomplete=lambda sweep, which, ordinal: (
        "cu_sweep ({} pipes) reached {} of {} CUs on hip device {}".format(
            which or "base", sweep.get("cus_covered"), sweep.get("cu_count"),
            ordinal)),
)


# ---- LDS sweep ----


def lds_sweep_enabled(lds_sweep: Optional[bool] = None) -> bool:
    """An explicit argument wins; None reads AMDXDP_LDS_SWEEP (unset, empty
    or 0 = off)."""
    return _switch_from_env(lds_sweep, LDS_SWEEP_ENV)


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


def run_lds_sweep(device: int = 0, mod=None) -> dict:
    """March test of the whole LDS of every CU of one HIP device."""
    if mod is None:
        mod = load_healthprobe(required=True)
    return mod.lds_sweep(device=device, corrupt=_lds_inject_from_env())


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


LDS_SWEEP = Sweep(
    key="lds_sweep", envs=(LDS_SWEEP_ENV, LDS_SWEEP_INJECT_ENV),
    ecc=("gfx", "gfx ", "sweep"), counts="cus",
    select=lambda arg: (None,) if lds_sweep_enabled(arg) else (),
    run=lambda device, mod, which: run_lds_sweep(device, mod),
    violations=lambda sweep, which: lds_sweep_violations(sweep),
    incomplete=lambda sweep, which: _incomplete_warning(
        "lds_sweep", sweep, simds=False),
)


def lds_sweep_with_ecc(device: int = 0, mod=None, sysroot: str = "/") -> dict:
    """run_lds_sweep between two readings of the GPU's gfx RAS counters.

    Adds `violations`, `warnings` and `ecc` (gfx_err_count before and after,
    None when unreadable) to the module's result: LDS is ECC-protected, so a
    weak cell may show only as a corrected error.
    """
    return check_sweep(LDS_SWEEP, device, None, mod, sysroot)[0]


# ---- VALU sweep ----


def valu_sweep_sets(valu_sweep=None) -> tuple:
    """The VALU op sets to sweep, in the order of VALU_SWEEP_SETS.  An
    explicit argument wins: False or True (none, all), "all", a comma list or
    an iterable of set names; None reads AMDXDP_VALU_SWEEP (unset, empty or
    0 = none, 1 or all = every set, otherwise a comma list)."""
    return _sets_from(valu_sweep, VALU_SWEEP_ENV, "valu_sweep", "op set",
                      VALU_SWEEP_SETS, switch=True)


def run_valu_sweep(device: int = 0, mod=None, op_set: str = "fma") -> dict:
    """Known-answer sweep of one VALU op set (VALU_SWEEP_SETS) over every CU
    and SIMD of one HIP device.  AMDXDP_VALU_SWEEP_INJECT="block:wave:op"
    simulates one bad op, named as in the module's tables."""
    if mod is None:
        mod = load_healthprobe(required=True)
    inject = _inject_from_env(
        VALU_SWEEP_INJECT_ENV, op_set, VALU_SWEEP_SETS,
        lambda s: [op["name"] for op in mod.valu_sweep_reference(s)["ops"]],
        "block:wave:op, op the name of an op of one of the sets")
    return mod.valu_sweep(device=device, inject=inject, op_set=op_set)


def valu_sweep_violations(sweep: dict, op_set: str = "") -> list:
    """One line per SIMD that failed the sweep of one set.  The scalar unit
    belongs to the CU: for set salu the SIMD is only where it was seen."""
    return _simd_violations("valu_sweep", sweep, "ops", ", ",
                            scalar=op_set == "salu")


def valu_sweep_incomplete_warning(sweep: dict, op_set: str):
    """The warning line of a set's sweep that found nothing bad but could
    not reach every SIMD, or None."""
    return _incomplete_warning("valu_sweep", sweep, op_set)


VALU_SWEEP = Sweep(
    key="valu_sweep", envs=(VALU_SWEEP_ENV, VALU_SWEEP_INJECT_ENV),
    sets=VALU_SWEEP_SETS, sets_key="valu_sweep", counts="simds",
    select=valu_sweep_sets,
    run=lambda device, mod, which: run_valu_sweep(device, mod, which),
    violations=valu_sweep_violations,
    incomplete=valu_sweep_incomplete_warning,
)


# ---- HBM scrub ----


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


def _check_hbm_scrub(device, mod, which):
    scrub = hbm_scrub(device, which, mod=mod)
    return scrub, scrub["violations"], scrub["warnings"]


# `which` is the byte count or "all"
HBM_SCRUB = Sweep(
    key="hbm_scrub", envs=(HBM_SCRUB_ENV,), ecc=("umc", "", "scrub"),
    select=lambda arg: tuple(
        b for b in [hbm_scrub_bytes_from_env(arg)] if b is not None),
    check=_check_hbm_scrub,
)


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
    kwargs = {} if patterns is None else {"patterns": list(patterns)}
    res, ecc_violations, ecc_warnings = _between_ecc_readings(
        HBM_SCRUB,
        lambda: mod.hbm_scrub(device=device, bytes=int(bytes), **kwargs),
        device, mod, sysroot)
    violations = hbm_scrub_violations(res) + ecc_violations
    warnings = []
    if whole and res["bytes_tested"] < HBM_SCRUB_FULL_SHARE * res["vram_bytes"]:
        warnings.append("hbm_scrub_partial: tested {} of {} bytes".format(
            res["bytes_tested"], res["vram_bytes"]))
    res["violations"] = violations
    res["warnings"] = warnings + ecc_warnings
    res["healthy"] = not violations
    return res


# ---- the deep probe ----

# in the order in which deep_health_probe runs them
SWEEPS = (CU_SWEEP, LDS_SWEEP, VALU_SWEEP, HBM_SCRUB)


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
    # or ValueError, before anything runs (the extra sets also while the CU
    # sweep is off); what else the environment chooses is read when its
    # sweep's turn comes
    if cu_sweep_extra is not None:
        cu_sweep_extra = cu_sweep_extra_sets(cu_sweep_extra)
    valu_sweep = valu_sweep_sets(valu_sweep)
    asked = {"cu_sweep": (cu_sweep, cu_sweep_extra), "lds_sweep": lds_sweep,
             "valu_sweep": valu_sweep, "hbm_scrub": hbm_scrub_bytes}
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
    warnings = []
    for sweep in SWEEPS:
        for which in sweep.select(asked[sweep.key]):
            # (the scrub reads its counters under /, whatever sysroot says)
            result, lines, warns = check_sweep(sweep, device, which, mod,
                                               sysroot)
            sweep.place(res, which, result)
            violations.extend(lines)
            warnings.extend(warns)
    if warnings:
        res["warnings"] = warnings
    res["floor_violations"] = violations
    if violations:
        res["healthy"] = False
    return res
