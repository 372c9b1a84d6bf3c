"""Static instruction counts of the tile loop of fused tile kernels, from the assembly `hipcc -S --cuda-device-only` writes.

    python tools/fused_tile_loop.py unit.s [substring of the mangled kernel name ...]

The tile loop of a kernel is delimited as the span of its WIDEST BACKWARD BRANCH: of all branches whose target label is defined
above them in the kernel's text, the one with the most instruction lines between label and branch (both included).  Every line
that is neither a label, a directive nor a comment counts as one instruction.  Classes: MFMA = v_mfma*; VALU = every other v_*
(v_readlane_b32 / v_writelane_b32 included); SALU = every s_* but s_nop, s_waitcnt and s_barrier (branches and scalar loads
included); one line per kernel as JSON."""
import json
import re
import sys


def kernels(text):
    cur, body = None, []
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end") or line.strip().startswith(".end_amdhsa_kernel"):
                yield cur, body
                cur = None
            else:
                body.append(line)


def tile_loop(body):
    ins, labels = [], {}
    for line in body:
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.?\w+):$", s)
        if m:
            labels[m.group(1)] = len(ins)
        elif not s.startswith("."):
            ins.append(s)
    best = (0, 0, 0)
    for i, s in enumerate(ins):
        m = re.match(r"^s_c?branch\w*\s+(\S+)$", s)
        if m and m.group(1) in labels and labels[m.group(1)] <= i and i + 1 - labels[m.group(1)] > best[0]:
            best = (i + 1 - labels[m.group(1)], labels[m.group(1)], i + 1)
    return ins[best[1]:best[2]]


def classify(loop):
    out = {"instructions": len(loop), "mfma": 0, "valu": 0, "readlane": 0, "writelane": 0, "salu": 0, "s_nop": 0, "s_waitcnt": 0,
           "s_barrier": 0, "s_load": 0, "lshl_add_u64": 0, "global_load": 0, "ds": 0}
    for s in loop:
        op = s.split()[0]
        if op.startswith("v_mfma"):
            out["mfma"] += 1
        elif op.startswith("v_"):
            out["valu"] += 1
            out["readlane"] += op.startswith("v_readlane")
            out["writelane"] += op.startswith("v_writelane")
            out["lshl_add_u64"] += op.startswith("v_lshl_add_u64")
        elif op in ("s_nop", "s_waitcnt", "s_barrier"):
            out[op] += 1
        elif op.startswith("s_"):
            out["salu"] += 1
            out["s_load"] += op.startswith("s_load") or op.startswith("s_buffer_load")
        elif op.startswith("global_load"):
            out["global_load"] += 1
        elif op.startswith("ds_"):
            out["ds"] += 1
    return out


if __name__ == "__main__":
    text = open(sys.argv[1]).read()
    for name, body in kernels(text):
        if len(sys.argv) > 2 and not any(k in name for k in sys.argv[2:]):
            continue
        print(json.dumps({"kernel": name, **classify(tile_loop(body))}))
