#!/usr/bin/env python3
"""Compare the kernels of two gfx950 listings of one unit (hipcc -S --cuda-device-only with the Makefile's flags, or the
.s files of `make asm`), kernel by kernel -- the listing rule of DESIGN.md section 19:

  a  symbol, kernarg bytes and static LDS bytes equal; private segment 0, no spill
  b  the ordered sequence of global_* and ds_* instructions equal (mnemonic plus the nt flag)
  c  VGPRs not above the parent's
  d  the multiset of v_* mnemonics equal

    tools/listing_diff.py PARENT.s BRANCH.s [--only SUBSTRING]

prints one markdown row per kernel (`ld<wr`: global loads in front of the first LDS write, parent/branch; `same`: the
streams are identical once labels are renumbered) and exits 1 when a kernel misses a, b, c or d.
"""
import collections
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta, cur = {}, None
    for line in text[text.index("amdhsa.kernels:"):].splitlines():
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    out = {}
    for name, k in meta.items():
        body = text[text.index("\n%s:" % name):]
        body = body[:body.index(".Lfunc_end")]
        ins, labels = [], {}
        for line in body.splitlines()[2:]:
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") or re.match(r"\.LBB\d+_\d+:", line):
                ins.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line))
        k["ins"] = ins
        ops = [(i.split()[0], " nt" if re.search(r"\bnt\b", i) else "") for i in ins if not i.endswith(":")]
        k["mem"] = [o + nt for o, nt in ops if o.startswith(("global_", "ds_"))]
        k["valu"] = collections.Counter(o for o, _ in ops if o.startswith("v_"))
        first_write = next((n for n, o in enumerate(k["mem"]) if o.startswith("ds_write")), len(k["mem"]))
        k["loads_first"] = sum(o.startswith("global_load") for o in k["mem"][:first_write])
        out[name] = k
    return out


def main():
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    parent, branch = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = subprocess.run(["c++filt"], input="\n".join(parent), capture_output=True, text=True).stdout.split("\n")
    print("| kernel | kernarg | LDS | VGPR | SGPR | instructions | ld<wr | a | b | c | d | same |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    bad = sorted(set(branch) - set(parent))
    for sym, nice in zip(parent, names):
        if only not in nice:
            continue
        p, b = parent[sym], branch.get(sym)
        if b is None:
            bad.append(sym)
            continue
        clean = all(k[f] == "0" for k in (p, b) for f in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
        a = clean and all(p[f] == b[f] for f in ("kernarg_segment_size", "group_segment_fixed_size"))
        checks = [a, p["mem"] == b["mem"], int(b["vgpr_count"]) <= int(p["vgpr_count"]), p["valu"] == b["valu"]]
        pair = lambda f: p[f] if p[f] == b[f] else "%s -> %s" % (p[f], b[f])
        n = (len(p["ins"]), len(b["ins"]))
        print("| `%s` | %s | %s | %s | %s | %s | %d / %d | %s | %s |" % (
            re.sub(r"^(void )?ghf::|\(.*$", "", nice), pair("kernarg_segment_size"), pair("group_segment_fixed_size"), pair("vgpr_count"),
            pair("sgpr_count"), n[0] if n[0] == n[1] else "%d -> %d" % n, p["loads_first"], b["loads_first"],
            " | ".join("ok" if c else "**NO**" for c in checks), "identical" if p["ins"] == b["ins"] else ""))
        if not all(checks):
            bad.append(sym)
            print("<!-- v_* parent - branch: %s; branch - parent: %s -->" % (dict(p["valu"] - b["valu"]), dict(b["valu"] - p["valu"])))
    if bad:
        sys.exit("kernels that miss a check or a partner: " + " ".join(bad))


if __name__ == "__main__":
    main()
