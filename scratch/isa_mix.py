"""Static instruction accounting of HIP kernels for gfx950, host only (no GPU needed).

    python scratch/isa_mix.py [--src FILE.hip] [--asm FILE.s] [--top N] [pattern ...]

Compiles FILE.hip (default: csrc/resblock_bf16.hip) to assembly with the flags of csrc/Makefile plus `--cuda-device-only -S`
(or reads a listing made that way with --asm) and prints, for every kernel whose mangled name contains one of the patterns
(default: the residual-block kernels of the update and the pair forwards):

  * next_free_vgpr, accum_offset, private_segment_fixed_size (scratch bytes) and the occupancy the compiler reports;
  * per basic block: VALU / MFMA / DS / VMEM / SALU / barrier counts, where the block branches to, its top VALU mnemonics;
  * which blocks form an ITEM LOOP: an outermost loop (a span of blocks closed by a backward branch) that holds MFMAs.  A kernel
    whose wave roles have loops of their own shows one item loop per role.  Blocks of loops nested inside are marked `+`
    (their counts are per trip of the inner loop, the sums below count them once);
  * per item loop the sum over its blocks, and v_mov / v_pk_max_i16 / address-arithmetic subtotals.

The counts are static: a block on a branch that one wave role never takes is still in the sum of a loop both roles share.

profiles/valu_diet_isa_after.txt is `python scratch/isa_mix.py` at the commit that holds it; profiles/valu_diet_isa_before.txt is the same
for its parent's source (the file may lie anywhere, csrc/ is on the include path):
    git show <parent>:train-procgen-pytorch_amd/csrc/resblock_bf16.hip > /tmp/parent/resblock_bf16.hip
    python scratch/isa_mix.py --src /tmp/parent/resblock_bf16.hip
"""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "train-procgen-pytorch_amd", "csrc")
DEFAULT_PATTERNS = ["resblock_bwd_full16d", "resblock_bwd_full32s", "resblock_bwd_full32q", "resblock_pair_bf16_kernel", "resblock_pair32r"]
ADDR_OPS = ("v_and_b32", "v_lshrrev_b32", "v_lshlrev_b32", "v_mul_u32_u24", "v_xor_b32", "v_mad_u32_u24", "v_lshl_add_u32", "v_add_u32", "v_or_b32",
            "v_and_or_b32", "v_lshl_or_b32", "v_mul_lo_u32", "v_bfe_u32", "v_add_lshl_u32", "v_sub_u32", "v_mad_u64_u32", "v_lshl_add_u64", "v_ashrrev_i32")


def makefile_flags(csrc=CSRC):
    """HIPCC, and CXXFLAGS with $(ARCH) filled in, as csrc/Makefile sets them (csrc: that directory of another checkout)."""
    var = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m and m.group(1) not in var:
            var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"])
    return os.environ.get("HIPCC", var.get("HIPCC", "hipcc")), flags.split()


def compile_to_asm(src, csrc=CSRC, extra=()):
    hipcc, flags = makefile_flags(csrc)
    fd, out = tempfile.mkstemp(suffix=".s")
    os.close(fd)
    cmd = [hipcc] + flags + list(extra) + ["-I", csrc, "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    text = open(out).read()
    os.unlink(out)
    return text


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_barrier":
        return "bar"
    if op.startswith("s_"):
        return "salu"
    return "other"


class Block:
    def __init__(self, name):
        self.name, self.cnt, self.valu, self.targets, self.falls = name, collections.Counter(), collections.Counter(), [], True


def parse_kernel(body):
    """Basic blocks of one function body in layout order.  A block starts at a label (.LBBf_n:) or at a `; %bb.n:` fall-through mark."""
    blocks = [Block("entry")]
    for raw in body.split("\n"):
        line = raw.strip()
        if not line:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line) or re.match(r"^; (%bb\.\d+):", line)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        if line.startswith((";", ".")):
            continue
        for piece in [p.strip() for p in line.split(";")[0].split("\n") if p.strip()]:
            op = piece.split()[0]
            b = blocks[-1]
            k = classify(op)
            b.cnt[k] += 1
            if k == "valu":
                b.valu[op] += 1
            if op.startswith("s_cbranch") or op == "s_branch":
                b.targets.append(piece.split()[-1])
                if op == "s_branch":
                    b.falls = False
            if op in ("s_endpgm", "s_setpc_b64"):
                b.falls = False
    return [b for b in blocks if sum(b.cnt.values()) or b.targets or b.name.startswith(".L")]


def loops_of(blocks):
    """(head, tail) index spans closed by a backward branch, merged per head; outermost ones and nesting depth per block."""
    idx = {b.name: k for k, b in enumerate(blocks)}
    span = {}
    for k, b in enumerate(blocks):
        for t in b.targets:
            if t in idx and idx[t] <= k:
                span[idx[t]] = max(span.get(idx[t], k), k)
    spans = sorted(span.items())
    changed = True
    while changed:                      # a span that crosses another one's end is one loop with it
        changed = False
        for a in range(len(spans)):
            for c in range(len(spans)):
                (h0, t0), (h1, t1) = spans[a], spans[c]
                if h0 < h1 <= t0 < t1:
                    spans[a] = (h0, t1); changed = True
    outer = [s for s in spans if not any(o != s and o[0] <= s[0] and s[1] <= o[1] for o in spans)]
    outer = sorted(set(outer))
    depth = [sum(1 for h, t in set(spans) if h <= k <= t) for k in range(len(blocks))]
    return outer, depth


def report(name, body, meta, top):
    blocks = parse_kernel(body)
    outer, depth = loops_of(blocks)
    item = [s for s in outer if sum(blocks[k].cnt["mfma"] for k in range(s[0], s[1] + 1)) > 0]
    print("=" * 150)
    print(name)
    print("  next_free_vgpr %s  accum_offset %s  private_segment_fixed_size %s  occupancy %s" % (
        meta.get("next_free_vgpr", "?"), meta.get("accum_offset", "?"), meta.get("private_segment_fixed_size", "?"), meta.get("occupancy", "?")))
    tot = collections.Counter()
    for b in blocks:
        tot.update(b.cnt)
    print("  whole kernel (static): VALU %d  MFMA %d  DS %d  VMEM %d  SALU %d  barrier %d" % tuple(tot[k] for k in ("valu", "mfma", "ds", "vmem", "salu", "bar")))
    print("  %-4s %-12s %5s %5s %5s %5s %5s %4s  %-26s %s" % ("loop", "block", "VALU", "MFMA", "DS", "VMEM", "SALU", "bar", "-> targets", "top VALU"))
    for k, b in enumerate(blocks):
        which = [n for n, s in enumerate(item) if s[0] <= k <= s[1]]
        if not which and not (b.cnt["valu"] + b.cnt["mfma"] + b.cnt["ds"] + b.cnt["vmem"] >= 8):
            continue                    # small blocks outside the item loops: prologue / epilogue plumbing
        mark = ("L%d" % which[0] + ("+" if depth[k] > 1 else "")) if which else ""
        tg = ",".join(t.replace(".LBB", "") for t in b.targets) + (",fall" if b.falls else "")
        tops = " ".join("%s:%d" % (o.replace("v_", "", 1), n) for o, n in b.valu.most_common(top))
        print("  %-4s %-12s %5d %5d %5d %5d %5d %4d  %-26s %s" % (mark, b.name.replace(".LBB", "BB"), b.cnt["valu"], b.cnt["mfma"], b.cnt["ds"], b.cnt["vmem"],
                                                                  b.cnt["salu"], b.cnt["bar"], tg[:26], tops))
    for n, (h, t) in enumerate(item):
        s, v = collections.Counter(), collections.Counter()
        for k in range(h, t + 1):
            s.update(blocks[k].cnt); v.update(blocks[k].valu)
        mov = sum(c for o, c in v.items() if o.startswith(("v_mov_b", "v_accvgpr")))
        addr = sum(c for o, c in v.items() if o.split("_e")[0] in ADDR_OPS or o in ADDR_OPS)
        print("  item loop L%d = %s .. %s (%d blocks%s): VALU %d  MFMA %d  DS %d  VMEM %d  SALU %d  barrier %d | v_mov/accvgpr %d  v_pk_max_i16 %d  integer/address ops %d" % (
            n, blocks[h].name.replace(".LBB", "BB"), blocks[t].name.replace(".LBB", "BB"), t - h + 1,
            ", inner loops inside" if any(depth[k] > 1 for k in range(h, t + 1)) else "",
            s["valu"], s["mfma"], s["ds"], s["vmem"], s["salu"], s["bar"], mov, v["v_pk_max_i16"], addr))
    if not item:
        print("  (no loop with MFMAs)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(CSRC, "resblock_bf16.hip"))
    ap.add_argument("--asm", help="read this listing instead of compiling --src")
    ap.add_argument("--top", type=int, default=6, help="VALU mnemonics shown per block")
    ap.add_argument("patterns", nargs="*", default=DEFAULT_PATTERNS)
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else compile_to_asm(a.src)
    print("# isa_mix: %s, gfx950, flags of csrc/Makefile; kernels matching %s" % (os.path.basename(a.asm or a.src), " | ".join(a.patterns)))
    metas = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        d = {k: v for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size) (\S+)", m.group(2))}
        o = re.search(r"; Occupancy: (\d+)", text[m.end():m.end() + 4000])
        if o:
            d["occupancy"] = o.group(1)
        metas[m.group(1)] = d
    found = 0
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        if any(p in m.group(1) for p in a.patterns):
            report(m.group(1), m.group(2), metas.get(m.group(1), {}), a.top)
            found += 1
    if not found:
        sys.exit("no kernel matches")


if __name__ == "__main__":
    main()
