"""Record the expected bits of the VALU sweep's set trans from the hardware.

    python -m k8s_device_plugin_amd.native.record_trans [--device N] > \
        k8s_device_plugin_amd/native/valu_trans_gfx950.inc

The low bits of v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32,
v_sin_f32 and v_rcp_f64 are not defined by IEEE 754, so the table's expected
words for them are what one wave of an MI355X gave for the table's operands
(valu_raw), in the order [op][test][lane][register].  The file's comment
carries, per op, the largest distance in ulp from the correctly rounded
value; tests/test_valu_sweep.py asserts exactly those.  A recording counts
only once valu_sweep(op_set="trans") passes with it on every SIMD of the card.
"""

from __future__ import annotations

import argparse
import math
import struct
import sys

# reference value of each op in double precision
TRANS_REFERENCE = {
    "v_exp_f32": lambda x: 2.0 ** x,
    "v_log_f32": lambda x: math.log2(x),
    "v_rcp_f32": lambda x: 1.0 / x,
    "v_rsq_f32": lambda x: 1.0 / math.sqrt(x),
    "v_sqrt_f32": lambda x: math.sqrt(x),
    "v_sin_f32": lambda x: math.sin(2.0 * math.pi * x),
    "v_rcp_f64": lambda x: 1.0 / x,
}


def _ordered(bits: int, width: int) -> int:
    """Sign-magnitude float bits -> an integer that orders like the value."""
    sign = 1 << (width - 1)
    return -(bits & (sign - 1)) if bits & sign else bits


def ulp_distance(name: str, operand_words, result_words) -> int:
    """Distance in units of the last place between the result an op gave
    and the correctly rounded value for that operand."""
    if name == "v_rcp_f64":
        x = struct.unpack("<d", struct.pack("<II", *operand_words))[0]
        want = struct.unpack("<Q", struct.pack("<d", TRANS_REFERENCE[name](x)))[0]
        got = result_words[1] << 32 | result_words[0]
        return abs(_ordered(got, 64) - _ordered(want, 64))
    x = struct.unpack("<f", struct.pack("<I", operand_words[0]))[0]
    # the double result rounded once to f32
    want = struct.unpack("<I", struct.pack("<f", TRANS_REFERENCE[name](x)))[0]
    return abs(_ordered(result_words[0], 32) - _ordered(want, 32))


def operands_of(ref: dict):
    """[(op descriptor, [per test: list of 64 operand-word tuples])]."""
    table = ref["table"]
    out = []
    for op in ref["ops"]:
        n_in = op["in_words"]
        tests = []
        for offset in op["offsets"]:
            words = struct.unpack_from(f"<{64 * n_in}I", table, offset)
            tests.append([words[l * n_in:(l + 1) * n_in] for l in range(64)])
        out.append((op, tests))
    return out


def max_ulp_per_op(ref: dict, recorded) -> dict:
    """Largest ulp distance of each op over the recorded words (a flat
    sequence in the file's order)."""
    worst = {}
    at = 0
    for op, tests in operands_of(ref):
        regs = op["regs"]
        worst[op["name"]] = 0
        for lanes in tests:
            for operand in lanes:
                d = ulp_distance(op["name"], operand, recorded[at:at + regs])
                worst[op["name"]] = max(worst[op["name"]], d)
                at += regs
    assert at == len(recorded)
    return worst


def record(mod, device: int = 0):
    """(words, {op: max ulp}) from one wave per test of every trans op."""
    ref = mod.valu_sweep_reference("trans")
    words = []
    for op, tests in operands_of(ref):
        for lanes in tests:
            a = b"".join(struct.pack(f"<{len(w)}I", *w) for w in lanes)
            out = mod.valu_raw(device, op["name"], a)
            words.extend(struct.unpack(f"<{64 * op['regs']}I", out))
    return words, max_ulp_per_op(ref, words)


def render(words, worst: dict) -> str:
    lines = [
        "// Expected result words of the VALU sweep's set trans, recorded from one",
        "// wave of an MI355X (gfx950) with valu_raw on the operands of valu_table.h:",
        "// [op][test][lane][register].  Written by",
        "// python -m k8s_device_plugin_amd.native.record_trans; do not edit.",
        "// Largest distance from the correctly rounded value, in ulp:",
    ]
    lines += [f"//   {name}: {ulp}" for name, ulp in worst.items()]
    for i in range(0, len(words), 8):
        lines.append(" ".join(f"0x{w:08x}u," for w in words[i:i + 8]))
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="record_trans", description=__doc__.split("\n")[0])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    try:  # torch's HIP runtime must load first (see __graft_entry__.build)
        import torch  # noqa: F401
    except ImportError:
        pass
    from . import load_healthprobe

    mod = load_healthprobe(required=True)
    words, worst = record(mod, args.device)
    sys.stdout.write(render(words, worst))
    return 0


if __name__ == "__main__":
    sys.exit(main())
