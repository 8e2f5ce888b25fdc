"""Are kernels' gfx950 assembly the same in two builds?

  hipcc ... --save-temps=obj -c csrc/ge_faml.hip     (once per build; writes
                                                      ge_faml-hip-amdgcn-amd-amdhsa-gfx950.s)
  python scripts/asm_identity.py OLD.s NEW.s faml_fast_repulse faml_sym_repulse

For every function whose mangled name contains one of the given substrings: the sha256
of its body in both files (basic-block labels renumbered: they carry the function's
ordinal in its file, and so does the padding before their comments) and `identical` or
`DIFFERENT`.  --loops prints, per function of
NEW.s, the self-looping basic blocks that hold a v_rsq_f64: instructions, fp64
instructions by opcode and ds_read count (a pair loop's cost per partner).
Exit status 1 if a function differs or is missing on one side.
"""
import hashlib
import re
import sys
from collections import Counter


def functions(path, keys):
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S*):[^\n]*\n", s, re.M):
        name = m.group(1)
        if any(k in name for k in keys):
            body = re.sub(r"BB\d+_", "BB_", s[m.end():s.index(".Lfunc_end", m.end())])
            # a label's comment is padded to a column: the padding follows the ordinal's digits
            out[name] = re.sub(r"^(\.LBB_\d+:)[ \t]+;", r"\1 ;", body, flags=re.M)
    return out


def pair_loops(body):
    blocks = re.split(r"^(\.LBB_\d+):.*\n", body, flags=re.M)
    out = []
    for i in range(1, len(blocks), 2):
        lab, txt = blocks[i], blocks[i + 1]
        if "v_rsq_f64" in txt and re.search(r"s_cbranch_\w+ %s\b" % re.escape(lab), txt):
            ins = [ln.split()[0] for ln in txt.splitlines()
                   if ln.strip() and not ln.strip().startswith((".", ";"))]
            out.append((len(ins), sorted(Counter(x for x in ins if "f64" in x).items()),
                        sum(x.startswith("ds_read") for x in ins)))
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--loops"]
    old, new, keys = args[0], args[1], args[2:]
    a, b = functions(old, keys), functions(new, keys)
    bad = 0
    for name in sorted(set(a) | set(b)):
        ha, hb = (hashlib.sha256(x.get(name, "").encode()).hexdigest()[:16] for x in (a, b))
        same = name in a and name in b and ha == hb
        bad += not same
        print(name, len(b.get(name, "").splitlines()), ha, hb, "identical" if same else "DIFFERENT")
    if "--loops" in sys.argv:
        for name in sorted(b):
            print(name, "pair loops:", pair_loops(b[name]))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main())
