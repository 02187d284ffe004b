"""Per-kernel VGPR / AGPR / scratch / LDS / occupancy from a hipcc -S listing: python tools/isa_stats.py [--hash] file.s [filter]
--hash: sorted by name, with a hash of each kernel's instruction text (from its symbol to its .Lfunc_end; comments
dropped, the function's number taken out of its block labels), so two listings compare per kernel with diff
whatever order their kernels come in."""
import hashlib
import re
import sys

KEYS = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")
args = [a for a in sys.argv[1:] if a != "--hash"]
want_hash = len(args) != len(sys.argv) - 1
cur = None
body = None
rows = []
for line in open(args[0]):
    m = re.match(r"^(_Z\w+):", line)
    if m:
        cur = {"name": m.group(1)}
        body = hashlib.sha256()
        rows.append(cur)
        continue
    if cur is None:
        continue
    if body is not None:
        if line.startswith(".Lfunc_end"):
            cur["hash"] = body.hexdigest()[:16]
            body = None
        else:
            text = re.sub(r"\.L(BB|tmp|func_begin)\d+", r".L\1", line.split(";")[0]).strip()
            if text:
                body.update(text.encode() + b"\n")
    for key in KEYS:
        m = re.match(r"^; %s: (\d+)" % key, line)
        if m and key not in cur:
            cur[key] = int(m.group(1))
flt = args[1] if len(args) > 1 else ""
if want_hash:
    rows.sort(key=lambda r: r["name"])
for r in rows:
    if flt in r["name"] and "NumVgprs" in r:
        print("%-70s vgpr %3d agpr %3d scratch %4d lds %6d occ %d%s" % (
            r["name"] if want_hash else r["name"][:70], r["NumVgprs"], r.get("NumAgprs", -1), r.get("ScratchSize", -1),
            r.get("LDSByteSize", -1), r.get("Occupancy", -1), "  " + r.get("hash", "-") if want_hash else ""))
