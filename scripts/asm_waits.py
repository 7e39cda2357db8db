"""Vector-memory loads and vmcnt waits of a kernel's tile loop (the label ..
backward branch span holding the most MFMAs, narrowest such span), in program
order, with the MFMAs between them counted.  Stores are left out unless
--stores is given.
usage: asm_waits.py file.s kernel_substring [--stores]"""
import re
import sys

path, ksub = sys.argv[1], sys.argv[2]
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and ksub in l)
end = next((i for i in range(start + 1, len(lines))
            if re.match(r"^_Z\S*:", lines[i]) or lines[i].startswith(".Lfunc_end")), len(lines))
body = lines[start:end]
labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\S+):", l)] if m}
best = None
for i, l in enumerate(body):
    m = re.search(r"s_cbranch\w*\s+(\.LBB\S+)", l) or re.search(r"s_branch\s+(\.LBB\S+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        a = labels[m.group(1)]
        nm = sum("v_mfma" in x for x in body[a:i + 1])
        if nm and (best is None or nm > best[0] or (nm == best[0] and i - a < best[2] - best[1])):
            best = (nm, a, i)
nm, a, b = best
code = [l.strip() for l in body if l.strip() and not l.strip().startswith(";") and not l.strip().startswith(".")]
loop = [l.strip() for l in body[a:b + 1] if l.strip() and not l.strip().startswith(";")]
print(f"kernel {body[0].rstrip(':')}")
print(f"tile loop {body[a].split(':')[0]}: {sum(1 for l in loop if not l.endswith(':'))} instructions, {nm} mfma; "
      f"whole kernel {len(code)} instructions")
mf = 0
pos = 0
for l in loop:
    if l.endswith(":"):
        continue
    pos += 1
    op = l.split()[0]
    if "v_mfma" in op:
        mf += 1
        continue
    vm = re.search(r"vmcnt\((\d+)\)", l)
    if op.startswith(("global_store", "buffer_store", "flat_store")) and "--stores" not in sys.argv:
        continue
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")) or (op == "s_waitcnt" and vm):
        what = f"s_waitcnt vmcnt({vm.group(1)})" if vm else " ".join(l.split()[:1] + [l.split()[-1] if "off" in l else ""])
        print(f"  {pos:5d}  after {mf:3d} mfma  {what.strip()}")
out = [l for l in code if l.split()[0].startswith("scratch_")]
print(f"scratch instructions in the kernel: {len(out)}, in the tile loop: "
      f"{sum(1 for l in loop if l.split()[0].startswith('scratch_'))}")
