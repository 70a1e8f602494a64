"""Compares two device listings of the library, function by function (no GPU).

A listing is what `hipcc -S --cuda-device-only` writes for bibim_renderer_amd/csrc/bibim_hip.hip with the Makefile's flags
(tests/test_kernel_resources.py makes one the same way).  Reported: the functions only one listing has; how many functions
have the same instruction stream once comments are stripped and block labels renumbered in order of appearance; and for every
function that differs its instruction count, vgpr_count, sgpr_count, private_segment_fixed_size (scratch) and
group_segment_fixed_size (LDS) on both sides.
usage: listing_compare.py A.s B.s"""
import re
import sys

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def functions(text):
    """name -> the function's lines: instructions and block labels, comments stripped, labels renumbered"""
    found = {}
    for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if name.startswith("."):
            continue
        labels, lines = {}, []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue  # blank, comment or directive
            lines.append(re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), line))
        found[name] = lines
    return found


def resources(text):
    """kernel name -> FIELDS, from the metadata at the end of the listing"""
    found = {}
    for block in re.split(r"\n  - (?=\.agpr_count:)", text[text.index("amdhsa.kernels:"):])[1:]:
        def field(key):
            return re.search(r"\n\s*\." + key + r":\s*(\S+)", "\n" + block).group(1)
        found[field("name")] = tuple(int(field(k)) for k in FIELDS)
    return found


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    texts = [open(p).read() for p in sys.argv[1:]]
    (fa, fb), (ra, rb) = map(functions, texts), map(resources, texts)
    for tag, mine, other in (("A", fa, fb), ("B", fb, fa)):
        for name in sorted(set(mine) - set(other)):
            print(f"only in {tag}: {name}")
    both = sorted(set(fa) & set(fb))
    differ = [n for n in both if fa[n] != fb[n]]
    print(f"{len(both)} functions in both listings, {len(both) - len(differ)} with identical instruction streams, {len(differ)} differ")
    print("# per differing function: instructions A -> B (B - A), then A -> B of " + ", ".join(FIELDS))
    for n in differ:
        ia, ib = (sum(not l.endswith(":") for l in f[n]) for f in (fa, fb))
        res = "  ".join(f"{x} -> {y}" for x, y in zip(ra[n], rb[n])) if n in ra and n in rb else "(no kernel metadata)"
        print(f"{n}\n    {ia} -> {ib} ({ib - ia:+d})   {res}")


if __name__ == "__main__":
    main()
