"""Instruction classes per basic block of one function in the compiler's
assembly output (hipcc -S --cuda-device-only ... -o file.s).

Classes, by mnemonic prefix only: branch (s_branch, s_cbranch_*, s_setpc,
s_swappc, s_call), nop (s_nop, s_sleep), wait (s_waitcnt*, s_barrier), salu
(any other s_*), lds (ds_*), vmem (global_*, buffer_*, flat_*, scratch_*),
valu (v_*), other.  A block starts at a label (.LBB*) or at a fall-through
block's comment (; %bb.N:) and ends at the next.

Usage: python scripts/asm_classes.py file.s <function substring> [--from LABEL --to LABEL] [--path A,B,..] [--moves]
  --from / --to   print only the blocks between two labels (inclusive) and their sum
  --path          print the named blocks in the order given (one traced path) and their sum
  --moves         add a column with the v_mov_b32 count of each block
The function substring selects the first symbol whose (mangled) name holds it.
"""
import argparse
import re
import sys

CLASSES = ("valu", "salu", "branch", "nop", "wait", "lds", "vmem", "other")


def classify(m):
    if m.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if m.startswith(("s_nop", "s_sleep")):
        return "nop"
    if m.startswith(("s_waitcnt", "s_barrier")):
        return "wait"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if m.startswith("v_"):
        return "valu"
    return "other"


def blocks_of(path, func):
    """[(label, {class: n}, n v_mov, [branch targets])] of the first function whose name holds func"""
    out, cur, inside = [], None, False
    label = re.compile(r"^([.\w$]+):")
    fall = re.compile(r"^; (%bb\.\d+):")
    for line in open(path):
        m = fall.match(line)
        if m and inside:
            cur = [m.group(1), dict.fromkeys(CLASSES, 0), 0, []]
            out.append(cur)
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip():
            continue
        m = label.match(s)
        if m:
            name = m.group(1)
            if not inside:
                if func in name and not name.startswith("."):
                    inside = True
                    cur = [name, dict.fromkeys(CLASSES, 0), 0, []]
                    out.append(cur)
                continue
            if name.startswith(".Lfunc_end"):
                break
            cur = [name, dict.fromkeys(CLASSES, 0), 0, []]
            out.append(cur)
            continue
        if not inside or s.lstrip().startswith("."):
            continue
        tok = s.split()
        mn = tok[0]
        c = classify(mn)
        cur[1][c] += 1
        if mn == "v_mov_b32_e32" or mn == "v_mov_b32":
            cur[2] += 1
        if c == "branch" and len(tok) > 1:
            cur[3].append(tok[-1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("function")
    ap.add_argument("--from", dest="first")
    ap.add_argument("--to", dest="last")
    ap.add_argument("--path")
    ap.add_argument("--moves", action="store_true")
    a = ap.parse_args()
    bl = blocks_of(a.asm, a.function)
    if not bl:
        sys.exit("no function with %r in its name" % a.function)
    names = [b[0] for b in bl]
    lo = names.index(a.first) if a.first else 0
    hi = names.index(a.last) if a.last else len(bl) - 1
    tot = dict.fromkeys(CLASSES, 0)
    mv = 0
    print("%-14s" % "block" + "".join("%7s" % c for c in CLASSES) + ("  v_mov" if a.moves else "") + "  -> targets")
    sel = bl[lo:hi + 1]
    if a.path:
        # a bare number N names the block .LBB<function>_N
        sel = [bl[names.index(n) if n.startswith(("%", ".")) else
                  next(i for i, x in enumerate(names) if x.startswith(".LBB") and x.endswith("_" + n))]
               for n in a.path.split(",")]
    for name, cnt, moves, tgt in sel:
        for c in CLASSES:
            tot[c] += cnt[c]
        mv += moves
        print("%-14s" % name[:14] + "".join("%7d" % cnt[c] for c in CLASSES) + ("%7d" % moves if a.moves else "") +
              "  " + " ".join(tgt))
    print("%-14s" % "sum" + "".join("%7d" % tot[c] for c in CLASSES) + ("%7d" % mv if a.moves else "") +
          "  (%d instructions)" % sum(tot.values()))


if __name__ == "__main__":
    main()
