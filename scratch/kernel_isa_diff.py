"""Kernel-by-kernel comparison of the device assembly of two source states, host only (no GPU needed).

    python scratch/kernel_isa_diff.py REV [expected-removal ...] [--added expected-addition ...] [--pair OLD=NEW ...]

Compiles every csrc/*.hip of the working tree and of git revision REV to gfx950 assembly (isa_mix.compile_to_asm: the flags of that
state's csrc/Makefile, plus the extra flags of a file's own rule in it, e.g. conv.o's; REV's sources and headers are unpacked into a
temporary directory).  Each listing is cut into kernels by mangled name -- the body from `NAME:` to `.Lfunc_end` and the kernel's
`.amdhsa_kernel ... .end_amdhsa_kernel` descriptor -- comments are dropped and the per-file numbering of local labels (.LBB<f>_<n>,
.Ltmp<n>, .Lfunc_end<f>, .LJTI<f>_<n>) is normalised, so a kernel that merely moved to another file compares equal.

Prints one line per kernel: `same`, `differs`, `only in REV` or `only in tree` (with the file(s) that hold it), and exits non-zero
unless every kernel is `same`, or is `only in REV` and matches an expected-removal argument, or is `only in tree` and matches an
expected-addition argument (each a substring of the mangled name; with none given, every `only in tree` fails).  A kernel
emitted by two files of one state is reported as an error.  That is a plain text comparison: it knows nothing about instructions.

`--pair OLD=NEW` (substrings that each name one kernel, OLD in REV and NEW in the tree) compares a rewritten kernel with the one it
replaces: identical text, or else the instruction count, the mnemonic histogram without the _e32 / _e64 encoding suffix,
next_free_vgpr, next_free_sgpr and private_segment_fixed_size (which must be 0) of both.  A pair that is neither identical nor equal in
all of these fails the run.  profiles/device_env_skeleton_isa.txt is the output for the commit that put the device envs on one skeleton.

profiles/misc_split_isa.txt is its output for the commit that split csrc/misc.hip, against that commit's parent.
"""
import concurrent.futures, glob, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import ROOT, CSRC, compile_to_asm

REL = os.path.relpath(CSRC, ROOT)


def extra_flags(csrc):
    """{"conv.hip": [flags]}: what a file's own rule in csrc/Makefile puts between $(CXXFLAGS) and -c."""
    extra, target = {}, None
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(\w+)\.o\s*:", line)
        if m:
            target = m.group(1) + ".hip"
        elif line.startswith("\t") and target:
            r = re.search(r"\$\(CXXFLAGS\)(.*?)\s-c\s", line)
            if r and r.group(1).split():
                extra[target] = r.group(1).split()
        elif line.strip():
            target = None
    return extra


def kernels_of(text):
    """{mangled name: normalised text} of one listing."""
    out = {}
    desc = {m.group(1): m.group(0) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", text, re.S)}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name = m.group(1)
        if name not in desc:
            continue
        tmp = {}
        lines = []
        for raw in (m.group(2) + desc[name]).split("\n"):
            line = raw.split(";")[0].rstrip()
            if not line.strip():
                continue
            line = re.sub(r"\.(LBB|LJTI)\d+_", r".\1_", line)
            line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)
            line = re.sub(r"\.Ltmp\d+", lambda t: tmp.setdefault(t.group(0), ".Ltmp#%d" % len(tmp)), line)
            lines.append(line)
        out[name] = "\n".join(lines)
    return out


def profile(text):
    """(instruction count, {mnemonic without _e32 / _e64: count}, {descriptor field: value}) of one normalised kernel text."""
    body, _, desc = text.partition(".amdhsa_kernel")
    hist = {}
    for line in body.split("\n"):
        w = line.split()
        if not w or w[0].startswith(".") or w[0].endswith(":"):
            continue
        m = re.sub(r"_e(32|64)$", "", w[0])
        hist[m] = hist.get(m, 0) + 1
    fields = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size)\s+(\S+)", desc))
    return sum(hist.values()), hist, fields


def compare_pair(spec, old, new):
    """Prints the comparison of one --pair; -> True if the new kernel meets the bar."""
    o_sub, _, n_sub = spec.partition("=")
    o, n = [k for k in old if o_sub in k], [k for k in new if n_sub in k]
    if len(o) != 1 or len(n) != 1:
        print("pair %s: names %d kernels in REV and %d in the tree (one each is needed)" % (spec, len(o), len(n)))
        return False
    print("pair %s -> %s" % (o[0], n[0]))
    if old[o[0]][0].replace(o[0], "K") == new[n[0]][0].replace(n[0], "K"):
        print("    identical text")
        return True
    (co, ho, fo), (cn, hn, fn) = profile(old[o[0]][0]), profile(new[n[0]][0])
    print("    instructions %d -> %d" % (co, cn))
    delta = ["%s %d -> %d" % (m, ho.get(m, 0), hn.get(m, 0)) for m in sorted(set(ho) | set(hn)) if ho.get(m, 0) != hn.get(m, 0)]
    print("    mnemonic histogram (without _e32 / _e64): " + ("same, %d mnemonics" % len(ho) if not delta else "DIFFERS: " + "; ".join(delta)))
    for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size"):
        print("    %s %s -> %s" % (k, fo.get(k), fn.get(k)))
    return co == cn and not delta and fo == fn and fn.get("private_segment_fixed_size") == "0"


def state(csrc, label):
    """{name: (text, [files])} over every .hip of one checkout's csrc/."""
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    extra = extra_flags(csrc)
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        texts = list(ex.map(lambda s: compile_to_asm(s, csrc, extra.get(os.path.basename(s), ())), srcs))
    ks, dup = {}, []
    for s, t in zip(srcs, texts):
        for name, body in kernels_of(t).items():
            if name in ks:
                ks[name][1].append(os.path.basename(s))
                dup.append("%s: %s is emitted by %s" % (label, name, " and ".join(ks[name][1])))
            else:
                ks[name] = (body, [os.path.basename(s)])
    return ks, dup


def main():
    if len(sys.argv) < 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    rev, expected, added, pairs = sys.argv[1], [], [], []
    into = expected
    for a in sys.argv[2:]:
        if a in ("--added", "--pair"):
            into = added if a == "--added" else pairs
        else:
            into.append(a)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, REL, "include"], stdout=subprocess.PIPE, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old, dup_old = state(os.path.join(tmp, REL), rev)
    new, dup_new = state(CSRC, "tree")
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], stdout=subprocess.PIPE, text=True, check=True).stdout.strip()
    print("# kernel_isa_diff: working tree against %s (%s); gfx950, flags of each state's csrc/Makefile" % (rev, sha))
    count, bad = {}, 0
    for name in sorted(set(old) | set(new)):
        if name in old and name in new:
            verdict = "same" if old[name][0] == new[name][0] else "differs"
            where = old[name][1][0] if old[name][1] == new[name][1] else "%s -> %s" % (old[name][1][0], new[name][1][0])
        elif name in old:
            verdict, where = "only in REV", old[name][1][0]
        else:
            verdict, where = "only in tree", new[name][1][0]
        count[verdict] = count.get(verdict, 0) + 1
        if (verdict == "differs" or (verdict == "only in REV" and not any(e in name for e in expected))
                or (verdict == "only in tree" and not any(e in name for e in added))):
            bad += 1
        print("%-12s %s  (%s)" % (verdict, name, where))
    for d in dup_old + dup_new:
        print("error: " + d)
    print("# " + ", ".join("%d %s" % (count[k], k) for k in ("same", "differs", "only in REV", "only in tree") if k in count))
    bad += sum(not compare_pair(p, old, new) for p in pairs)
    sys.exit(1 if bad or dup_old or dup_new else 0)


if __name__ == "__main__":
    main()
