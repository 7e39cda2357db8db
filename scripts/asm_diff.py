"""Kernel-by-kernel comparison of two device assembly listings (hipcc ... --cuda-device-only -S).
usage: python scripts/asm_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] [--rename REGEX=REPL ...] [--lines N]

Each function's body (label to .Lfunc_end) is keyed by its mangled name, comments and
directives dropped, the function index in .LBB<n>_<m> labels renumbered; kernels also
carry their metadata (.vgpr_count, .sgpr_count, .private_segment_fixed_size,
.group_segment_fixed_size, accum offset).  Prints: functions in old, in new, identical,
removed, added, and for every differing one the differing lines (at most N, default 40).
--rename (re.sub on the old mangled names) compares a renamed kernel, such as an
instance of a folded template, against its old instance."""
import difflib
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def parse(paths):
    funcs = {}
    for path in paths.split(","):
        lines = open(path).read().split("\n")
        name, body = None, []
        entry = {}  # the amdhsa.kernels item being read

        def commit():
            if entry.get(".name") in funcs:
                funcs[entry[".name"]]["meta"].update({k: v for k, v in entry.items() if k in META})

        for l in lines:
            if name is None:
                m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
                if m:
                    name, body = m.group(1), []
                    funcs[name] = {"body": body, "kernel": False, "meta": {}}
                    continue
                m = re.match(r"^  (- |  )(\.[a-z_]+):\s+(\S+)$", l)  # item keys; .args entries sit deeper
                if m:
                    if m.group(1) == "- ":
                        commit()
                        entry = {}
                    entry[m.group(2)] = m.group(3)
                elif l.startswith("amdhsa.target"):
                    commit()
                    entry = {}
                continue
            s = l.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                name = None
                continue
            m2 = re.match(r"\.amdhsa_accum_offset\s+(\d+)", s)
            if m2:
                funcs[name]["meta"]["accum_offset"] = m2.group(1)
            if s.startswith(".amdhsa_kernel"):
                funcs[name]["kernel"] = True
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return funcs


def main():
    args = sys.argv[1:]
    rename, nlines, pos = [], 40, []
    i = 0
    while i < len(args):
        if args[i] == "--rename":
            rename.append(args[i + 1].split("=", 1))
            i += 2
        elif args[i] == "--lines":
            nlines = int(args[i + 1])
            i += 2
        else:
            pos.append(args[i])
            i += 1
    old, new = parse(pos[0]), parse(pos[1])
    back = {}
    for k in list(old):
        n = k
        for rx, repl in rename:
            n = re.sub(rx, repl, n)
        if n != k:
            old[n] = old.pop(k)
            back[n] = k
    nk = lambda f: sum(1 for v in f.values() if v["kernel"])
    same = [k for k in old if k in new and old[k]["body"] == new[k]["body"] and old[k]["meta"] == new[k]["meta"]]
    diff = [k for k in old if k in new and k not in same]
    removed = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"old: {len(old)} functions, {nk(old)} kernels; new: {len(new)} functions, {nk(new)} kernels")
    print(f"identical {len(same)} (renamed among them {sum(1 for k in same if k in back)}), "
          f"differing {len(diff)}, removed {len(removed)}, added {len(added)}")
    for k in removed:
        print("removed", k)
    for k in added:
        print("added  ", k)
    for k in diff:
        a, b = old[k], new[k]
        print(f"differs {k}" + (f" (old name {back[k]})" if k in back else ""))
        print(f"  instructions and labels: {len(a['body'])} -> {len(b['body'])}; metadata "
              + ("equal" if a["meta"] == b["meta"] else f"{a['meta']} -> {b['meta']}"))
        d = [l for l in difflib.unified_diff(a["body"], b["body"], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        # the vector, LDS and memory instructions alone, scalar register names masked: equal
        # when only the kernel-argument layout and the scalar allocation moved
        vec = lambda f: [re.sub(r"\bs\d+\b|\bs\[\d+:\d+\]", "S", l) for l in f["body"] if not l.startswith(("s_", ".LBB"))]
        print(f"  {len(d)} differing lines; non-scalar instructions with SGPR names masked: "
              + ("equal" if vec(a) == vec(b) else "differ"))
        for l in d[:nlines]:
            print("   ", l)
    return 0


if __name__ == "__main__":
    sys.exit(main())
