"""Compares two gfx950 assembly listings of one translation unit kernel by kernel (dev tool; no GPU needed).

    hipcc <the Makefile's FLAGS> --cuda-device-only -S engine.hip -o parent.s     (in the parent's tree, and in this one -> new.s)
    python tools/codeobj_ab.py parent.s new.s [more pairs ...] > profiles/rNN/vK_codeobj_ab.txt

Kernels whose name contains "mid8" or "strided_pass" (the fused middles and the strided passes of ntt_kernels.hpp: the he_mul core) are compared
by resources and instruction counts, one row each; scalar instructions may differ there and are listed.  Every other kernel must have the same instruction sequence, opcodes and operands.
Exit status 1 when a kernel is missing on one side, a sequence differs, or a count of a mid8 kernel does."""
import re, subprocess, sys

META = (".vgpr_count", ".vgpr_spill_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
COUNTS = (("valu", r"v_"), ("mad64", r"v_mad_u64_u32"), ("ds", r"ds_"), ("vmem", r"global_|buffer_"), ("scratch", r"scratch_"), ("branch", r"s_cbranch|s_branch"),
          ("cndmask", r"v_cndmask"), ("salu", r"s_"))


def kernels(path):
    text = open(path).read()
    meta = {}
    for block in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        sym = re.search(r"^\s+\.symbol:\s+'?([^\s']+)\.kd", block, flags=re.M)
        if sym:
            meta[sym.group(1)] = tuple(int(re.search(r"^\s*%s:\s+(\d+)" % re.escape(f), block, flags=re.M).group(1)) for f in META)
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.M | re.S):
        if m.group(1) not in meta:
            continue
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", l.split(";")[0].strip())) for l in m.group(2).split("\n")]
        out[m.group(1)] = (meta[m.group(1)], [l for l in ins if l and not l.startswith(".") or l.startswith(".LBB")])
    return out


def main():
    bad = 0
    print("# %s" % " ".join(META))
    print("# counts: %s  (parent -> new where they differ)" % " ".join(c for c, _ in COUNTS))
    for pa, pb in zip(sys.argv[1::2], sys.argv[2::2]):
        a, b = kernels(pa), kernels(pb)
        names = subprocess.run(["c++filt"], input="\n".join(sorted(set(a) | set(b))), capture_output=True, text=True).stdout.split("\n")
        same = 0
        rows = []
        for sym, name in zip(sorted(set(a) | set(b)), names):
            if sym not in a or sym not in b:
                bad += 1
                rows.append("MISSING in %s: %s" % ("parent" if sym not in a else "new", name))
            elif "mid8" not in sym and "strided_pass" not in sym:
                if a[sym] == b[sym]:
                    same += 1
                else:
                    bad += 1
                    rows.append("DIFFERS: %s" % name)
            else:
                cnt = [[sum(1 for l in k[sym][1] if re.match(pat, l)) for _, pat in COUNTS] for k in (a, b)]
                ok = a[sym][0] == b[sym][0] and cnt[0][:-1] == cnt[1][:-1]
                bad += not ok
                show = lambda x, y: str(x) if x == y else "%s->%s" % (x, y)
                rows.append("%-4s %s | %s | salu diff %+d | %s" % ("ok" if ok else "FAIL", " ".join(show(x, y) for x, y in zip(a[sym][0], b[sym][0])),
                                                             " ".join(show(x, y) for x, y in zip(cnt[0], cnt[1])), cnt[1][-1] - cnt[0][-1],
                                                             re.sub(r"^void gpq::|\(.*$", "", name)))
        print("\n## %s: %d kernels on each side; %d others with identical instruction sequences" % (pb.split("/")[-1], len(a), same))
        print("\n".join(rows))
    print("\n%s" % ("ALL CHECKS HOLD" if not bad else "%d FAILURES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
