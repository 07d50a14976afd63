"""Per-kernel fingerprint of a directory of device assembly files (``hipcc ... --offload-device-only -S``), and the comparison
of two such directories: the check that a host-side refactor left every kernel alone.

    python tools/kernel_fingerprint.py DIR                 # the table: one line per kernel
    python tools/kernel_fingerprint.py PARENT_DIR NEW_DIR  # the comparison (exit status 1 when names or metadata differ)

A kernel is keyed by its mangled name (``.amdhsa_kernel NAME``) and de-duplicated across translation units.  Compared: the set
of names; each kernel's metadata (VGPR / AGPR / SGPR counts, private and group segment sizes, spill counts, kernarg size, from
the ``amdhsa.kernels`` notes); and a SHA-256 of its instruction text with comments dropped and the function-numbered local
labels (``.LBB<n>_<m>``, ``.Ltmp``, ``.Lfunc_end<n>``) renumbered in order of appearance - they change when a kernel moves to
another translation unit.  Text and metadata only: nothing is executed.
"""
import glob
import hashlib
import os
import re
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count", "kernarg_segment_size")
_LABEL = re.compile(r"\.L(?:BB|tmp|func_end|func_begin|JTI|CPI)[0-9_]+")


def _normalised(lines):
    names = {}

    def ren(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))

    out = []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()       # comments carry file-local numbering as well
        if not line.strip() or line.lstrip().startswith((".file", ".loc", ".cfi", ".p2align", ".section", ".type", ".size", ".globl",
                                                          ".weak", ".protected", ".hidden", ".text", ".ident", ".addrsig")):
            continue
        out.append(_LABEL.sub(ren, line))
    return "\n".join(out)


def read_dir(path):
    """{mangled name: {"meta": {...}, "text": sha256, "units": [file, ...]}}"""
    kernels = {}
    for fn in sorted(glob.glob(os.path.join(path, "*.s"))):
        unit = os.path.basename(fn)
        with open(fn) as f:
            lines = f.read().split("\n")
        declared = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
        # instruction text: from the kernel's label to its .Lfunc_end
        i = 0
        while i < len(lines):
            m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
            if m and m.group(1) in declared:
                j = i + 1
                while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                    j += 1
                k = kernels.setdefault(m.group(1), {"meta": {}, "text": None, "units": []})
                digest = hashlib.sha256(_normalised(lines[i + 1:j]).encode()).hexdigest()
                if k["text"] not in (None, digest):
                    k["text"] = "differs between translation units"
                else:
                    k["text"] = digest
                k["units"].append(unit)
                i = j
            i += 1
        # metadata: the YAML notes at the end of the file, one list entry ("  - .key: value", then "    .key: value") per kernel
        entry = None
        for line in lines + ["  - .end: 0"]:
            m = re.match(r"^  (- | )\s*\.(\w+):\s*(.*)$", line)
            if not m:
                continue
            if m.group(1) == "- ":
                name = (entry or {}).get("symbol", "")
                name = name[:-3] if name.endswith(".kd") else name
                if name in kernels:
                    meta = {k: int(entry.get(k, 0)) for k in META}
                    if kernels[name]["meta"] not in ({}, meta):
                        meta["differs_between_units"] = 1
                    kernels[name]["meta"] = meta
                entry = {}
            if entry is not None:
                entry[m.group(2)] = m.group(3).strip().strip("'")
    return kernels


def table(kernels):
    rows = []
    for name in sorted(kernels):
        k = kernels[name]
        rows.append("%s %s text=%s" % (name, " ".join("%s=%d" % (m, k["meta"].get(m, -1)) for m in META), k["text"][:16]))
    return rows


def main(argv):
    if len(argv) == 2:
        print("\n".join(table(read_dir(argv[1]))))
        return 0
    old, new = read_dir(argv[1]), read_dir(argv[2])
    rc = 0
    print("kernels: %d before, %d after" % (len(old), len(new)))
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print("names only before: %d, only after: %d" % (len(gone), len(added)))
    for n in gone:
        print("  - " + n)
    for n in added:
        print("  + " + n)
    rc |= bool(gone or added)
    meta = [n for n in sorted(set(old) & set(new)) if old[n]["meta"] != new[n]["meta"]]
    print("metadata differs (%s): %d" % (", ".join(META), len(meta)))
    for n in meta:
        print("  %s\n    before %r\n    after  %r" % (n, old[n]["meta"], new[n]["meta"]))
    rc |= bool(meta)
    text = [n for n in sorted(set(old) & set(new)) if old[n]["text"] != new[n]["text"]]
    print("instruction text differs (labels renumbered, comments dropped): %d" % len(text))
    for n in text:
        print("  %s  %s -> %s  (%s -> %s)" % (n, old[n]["text"][:16], new[n]["text"][:16], ",".join(old[n]["units"]), ",".join(new[n]["units"])))
    moved = [n for n in sorted(set(old) & set(new)) if old[n]["units"] != new[n]["units"]]
    print("kernels compiled in another translation unit than before: %d" % len(moved))
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv))
