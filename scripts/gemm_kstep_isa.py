"""Per-path instruction accounting of a persistent GEMM kernel's K-tile body (CPU only).

Reads the gfx950 assembly of one kernel instantiation (a `hipcc -S` file, or compiles
boxfusion_amd/csrc/bf_gemm.hip itself), rebuilds its control-flow graph and walks the K loop.  A
K-tile is the stretch between eight consecutive s_barrier: phases P1..P4, each a memory section
(up to the phase's first barrier) and an MFMA section (between its two barriers); what follows the
eighth barrier (walk bookkeeping) is charged to the next K-tile's P1 memory section, where it runs.

Reported paths, each the shortest feasible-looking path of its kind through the loop(s):
  steady  a K-tile that issues no global store (neither first nor last of a tile), taken from the
          innermost loop that holds barriers
  first   a K-tile with stores in P1 only (the previous tile's last quadrant)
  last    a K-tile with stores in each of P2, P3, P4 (the epilogues of its own tile)
  other   store-free K-tile bodies outside the innermost loop (peeled bodies), if any
Branches on EXEC (lane masks) are taken as fall-through: the guarded instructions issue whenever
one lane is active.  Scalar branches are enumerated both ways.

usage: gemm_kstep_isa.py [--asm file.s] [--kernel k_gemm256q] INST [INST ...]
  INST: qkv | fc1 | res | proj | a mangled template-argument string such as ILb1ELi1ELb0ELi0ELi4E
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "boxfusion_amd", "csrc", "bf_gemm.hip")
# k_gemm256q<OUT_BF16, ACT, RES, F8, MB1> at 256-row tiles
NAMED = {"qkv": "ILb1ELi0ELb0ELi0ELi4E", "fc1": "ILb1ELi1ELb0ELi0ELi4E", "res": "ILb0ELi0ELb1ELi0ELi4E",
         "proj": "ILb0ELi0ELb1ELi0ELi4E"}
CLASSES = ["MFMA", "ds_read", "ds_write", "LDS-DMA", "vmem", "VALU", "trans", "SALU", "smem", "wait", "barrier", "nop"]
TRANS = ("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq", "v_sin", "v_cos")
SECTIONS = ["P1 mem", "P1 mfma", "P2 mem", "P2 mfma", "P3 mem", "P3 mfma", "P4 mem", "P4 mfma"]
MAX_PATHS = 400000


def classify(op, text):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_"):
        return "ds_write"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        if re.search(r"\blds\b", text) or "_lds_" in op:
            return "LDS-DMA"
        return "vmem"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op == "s_barrier":
        return "barrier"
    if op in ("s_nop", "s_sleep"):
        return "nop"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    return "SALU"


def kernel_lines(asm, kernel, inst):
    lines = open(asm).read().split("\n")
    pat = re.compile(r"^_Z\d+" + re.escape(kernel) + re.escape(inst) + r"\w*:")
    start = [i for i, l in enumerate(lines) if pat.match(l)]
    if not start:
        raise SystemExit(f"no kernel {kernel}{inst} in {asm}")
    end = next(i for i in range(start[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start[0]].split(":")[0], lines[start[0] + 1:end]


class Block:
    def __init__(self, name):
        self.name, self.ins, self.succ = name, [], []


def build_cfg(body):
    """basic blocks in layout order; ins = [(class, stores)], succ = [(block index, kind)]"""
    blocks, pending = [Block("entry")], []
    cur = blocks[0]
    for raw in body:
        l = raw.split(";")[0].rstrip()
        if not l.strip():
            continue
        m = re.match(r"^(\.?[\w$.]+):", l)
        if m:
            cur = Block(m.group(1))        # empty blocks (label after label) just fall through
            blocks.append(cur)
            continue
        t = l.strip()
        if t.startswith("."):
            continue
        op = t.split()[0]
        if op.startswith("s_cbranch") or op == "s_branch":
            cur.ins.append(("SALU", False))
            pending.append((cur, op, t.split()[-1]))
            nb = Block(cur.name + "+")
            blocks.append(nb)
            cur = nb
            continue
        if op == "s_endpgm":
            cur.ins.append(("SALU", False))
            pending.append((cur, op, None))
            nb = Block(cur.name + "+")
            blocks.append(nb)
            cur = nb
            continue
        cur.ins.append((classify(op, t), "store" in op))
    index = {b.name: i for i, b in enumerate(blocks)}
    term = {id(b): (op, tgt) for b, op, tgt in pending}
    for i, b in enumerate(blocks):
        op, tgt = term.get(id(b), (None, None))
        if op == "s_endpgm":
            continue
        if op == "s_branch":
            b.succ.append((index[tgt], "jump"))
            continue
        if op is not None:
            exec_branch = "exec" in op
            if not exec_branch:
                b.succ.append((index[tgt], "taken"))
            elif index[tgt] <= i:
                b.succ.append((index[tgt], "taken"))      # a loop on EXEC (waterfall): keep the back edge
        if i + 1 < len(blocks):
            b.succ.append((i + 1, "fall"))
    return blocks


def loops_of(blocks):
    """natural loops from layout back edges: {header: set(blocks)}"""
    pred = collections.defaultdict(list)
    for i, b in enumerate(blocks):
        for s, _ in b.succ:
            pred[s].append(i)
    loops = {}
    for u, b in enumerate(blocks):
        for h, _ in b.succ:
            if h <= u:
                body, stack = {h, u}, [u]
                while stack:
                    x = stack.pop()
                    if x == h:
                        continue
                    for p in pred[x]:
                        if p not in body and p >= h:
                            body.add(p)
                            stack.append(p)
                loops.setdefault(h, set()).update(body)
    return loops


def block_pieces(b):
    """the block's instructions cut at its barriers: [Counter, ...] (n barriers -> n + 1 pieces)"""
    pieces = [collections.Counter()]
    for cls, st in b.ins:
        pieces[-1][cls] += 1
        if st:
            pieces[-1]["store"] += 1
        if cls == "barrier":
            pieces.append(collections.Counter())
    return pieces


def loop_paths(blocks, h, body, pieces):
    """cyclic paths header -> back edge inside `body` (inner back edges not taken), as piece lists"""
    out, stack, n = [], [(h, (h,))], 0
    while stack:
        x, path = stack.pop()
        succ = [s for s, _ in blocks[x].succ]
        closed = False
        for s in succ:
            if s == h:
                closed = True
            elif s in body and s > x:          # forward edges only: inner loops run once
                stack.append((s, path + (s,)))
        if closed:
            n += 1
            if n > MAX_PATHS:
                raise SystemExit("too many paths")
            seq = [collections.Counter()]
            for bi in path:
                ps = pieces[bi]
                seq[-1] = seq[-1] + ps[0]
                seq.extend(ps[1:])
            out.append(seq)
    return out


def segments(seq):
    """cut a cyclic piece sequence into K-tiles of 8 barriers: [[8 section Counters], ...]"""
    nb = len(seq) - 1
    if nb == 0 or nb % 8:
        return []
    segs = []
    for k in range(nb // 8):
        sec = [collections.Counter(seq[k * 8 + j]) for j in range(8)]
        sec[0] = sec[0] + (seq[nb] if k == 0 else collections.Counter())   # the wrap-around tail
        segs.append(sec)
    return segs


def kind_of(sec):
    """a last K-tile stores in P2, P3 and P4 alike (the kernel tests the one condition in each of
    them: paths that take some of those arms only cannot run and are dropped)"""
    s0 = sec[0]["store"]
    s1 = [sec[j]["store"] > 0 for j in (2, 4, 6)]
    if s0 == 0 and not any(s1):
        return "steady"
    if not any(s1):
        return "first"
    return "last" if s0 == 0 and all(s1) else "infeasible"


def total(sec):
    return sum(v for c in sec for k, v in c.items() if k != "store")


def sig(sec):
    return tuple(tuple(c.get(k, 0) for k in CLASSES) for c in sec)


def report(title, sec, nvar, out):
    out.append(f"  {title}: {total(sec)} instructions ({nvar} path variant{'s' if nvar != 1 else ''} of this kind, the shortest shown)")
    out.append("    " + f"{'section':8s}" + "".join(f"{c:>9s}" for c in CLASSES) + f"{'total':>9s}")
    tot = collections.Counter()
    for name, c in zip(SECTIONS, sec):
        out.append("    " + f"{name:8s}" + "".join(f"{c.get(k, 0):9d}" for k in CLASSES) + f"{sum(c.get(k, 0) for k in CLASSES):9d}")
        tot.update({k: c.get(k, 0) for k in CLASSES})
    mem = collections.Counter()
    for j in (0, 2, 4, 6):
        mem.update({k: sec[j].get(k, 0) for k in CLASSES})
    out.append("    " + f"{'all mem':8s}" + "".join(f"{mem.get(k, 0):9d}" for k in CLASSES) + f"{sum(mem.values()):9d}")
    out.append("    " + f"{'K-tile':8s}" + "".join(f"{tot.get(k, 0):9d}" for k in CLASSES) + f"{sum(tot.values()):9d}")


def analyse(asm, kernel, inst):
    sym, body = kernel_lines(asm, kernel, inst)
    blocks = build_cfg(body)
    pieces = [block_pieces(b) for b in blocks]
    loops = {h: bs for h, bs in loops_of(blocks).items() if sum(len(pieces[b]) - 1 for b in bs) >= 8}
    out = [f"{sym}", f"  {sum(len(b.ins) for b in blocks)} instructions, {len(blocks)} basic blocks, "
           f"{len(loops)} loop(s) with K-tile barriers"]
    if not loops:
        return out + ["  no K loop found"]
    inner = [h for h in loops if not any(o != h and loops[o] < loops[h] for o in loops)]
    found = collections.defaultdict(dict)       # kind -> {signature: sections}
    for h, bs in loops.items():
        for seq in loop_paths(blocks, h, bs, pieces):
            for sec in segments(seq):
                k = kind_of(sec)
                if k == "steady" and h not in inner:
                    k = "other"
                found[k][sig(sec)] = sec
    inner_steady = set(found["steady"])
    found["other"] = {s: v for s, v in found["other"].items() if s not in inner_steady}
    names = {"steady": "steady K-tile (innermost loop)", "first": "first K-tile of a tile",
             "last": "last K-tile of a tile", "other": "store-free K-tile outside the innermost loop"}
    for k in ("steady", "first", "last", "other"):
        if found[k]:
            report(names[k], min(found[k].values(), key=total), len(found[k]), out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--kernel", default="k_gemm256q")
    ap.add_argument("inst", nargs="+")
    a = ap.parse_args()
    asm = a.asm
    tmp = None
    if not asm:
        tmp = tempfile.mkdtemp()
        asm = os.path.join(tmp, "bf_gemm.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fPIC",
                        "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-S", "--cuda-device-only", "-o", asm, SRC],
                       check=True, stderr=subprocess.DEVNULL)
    print("# K-tile instruction accounting (scripts/gemm_kstep_isa.py): gfx950, hipcc -O3")
    for inst in a.inst:
        print("\n".join(analyse(asm, a.kernel, NAMED.get(inst, inst))))
        print()
    if tmp:
        os.remove(asm)
        os.rmdir(tmp)


if __name__ == "__main__":
    sys.exit(main())
