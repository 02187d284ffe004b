"""Instruction classes per basic block of a kernel in a hipcc -S listing, and their sum along a block path:
    python tools/block_path.py file.s KERNEL [--path 0,3,7,7,9] [--blocks]
KERNEL: a substring of the mangled name (the first match).  A block is named by its number: block 0 is the entry,
block N the label .LBB<fn>_N.  --path sums the listed blocks in order, a block counted as often as it is listed
(a loop block once per trip); without it every block is summed once (the static text).  --blocks prints the table
per block as well.  Classes, by mnemonic prefix:
    matrix     v_mfma_*, v_smfmac_*
    lane-move  v_readlane_*, v_writelane_*, v_readfirstlane_*
    vector     every other v_*
    LDS        ds_*
    memory     global_*, buffer_*, flat_*, scratch_*, s_load_*, s_buffer_load_*
    scalar     every other s_*
    wait       s_waitcnt*, s_barrier (counted in scalar too)
"""
import re
import sys

CLASSES = ("vector", "lane-move", "matrix", "LDS", "memory", "scalar", "wait", "all")


def classify(op):
    if op.startswith(("v_mfma_", "v_smfmac_")):
        return ("matrix",)
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return ("lane-move",)
    if op.startswith("v_"):
        return ("vector",)
    if op.startswith("ds_"):
        return ("LDS",)
    if op.startswith(("global_", "buffer_", "flat_", "scratch_", "s_load_", "s_buffer_load_")):
        return ("memory",)
    if op.startswith(("s_waitcnt", "s_barrier")):
        return ("scalar", "wait")
    if op.startswith("s_"):
        return ("scalar",)
    return ()


def blocks_of(path, want):
    """[(block number, {class: count})] of the first kernel whose name contains `want`, in text order."""
    name, blocks, cur = None, [], None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            if name:
                break
            if want in m.group(1):
                name = m.group(1)
                cur = {c: 0 for c in CLASSES}
                blocks.append((0, cur))
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = re.match(r"^\.LBB\d+_(\d+):", line)
        if m:
            cur = {c: 0 for c in CLASSES}
            blocks.append((int(m.group(1)), cur))
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith(".") or text.endswith(":"):
            continue
        op = text.split()[0]
        cls = classify(op)
        if cls:
            cur["all"] += 1
            for c in cls:
                cur[c] += 1
    return name, blocks


def row(label, cnt):
    return "%-14s" % label + "".join("%10d" % cnt[c] for c in CLASSES)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = None
    if "--path" in sys.argv:
        path = [int(v) for v in sys.argv[sys.argv.index("--path") + 1].split(",")]
        args.remove(sys.argv[sys.argv.index("--path") + 1])
    name, blocks = blocks_of(args[0], args[1])
    if name is None:
        sys.exit("no kernel matching %r in %s" % (args[1], args[0]))
    by_no = dict(blocks)
    print(name)
    print("%-14s" % "block" + "".join("%10s" % c for c in CLASSES))
    if "--blocks" in sys.argv:
        for no, cnt in blocks:
            print(row(no, cnt))
    walk = path if path is not None else [no for no, _ in blocks]
    total = {c: sum(by_no[no][c] for no in walk) for c in CLASSES}
    print(row("path (%d)" % len(walk) if path is not None else "static (%d)" % len(walk), total))


if __name__ == "__main__":
    main()
