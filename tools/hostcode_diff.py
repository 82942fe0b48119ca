#!/usr/bin/env python3
"""Did a change to the host launchers change their host object code?  For a change meant to leave
launch cost alone; the companion of devcode_same.sh for the host side, no GPU needed.
    tools/hostcode_diff.py <git-rev>
Compiles csrc/cog_engine.hip host-only (build_ext._compile_cmd's flags) from an export of <git-rev>
and from the working tree, disassembles both objects and prints, per function of namespace cog, the
instruction count on each side (padding nops left out) and whether the instruction text is the same
once addresses, symbol offsets and relocation addends are dropped."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPILE = ("import subprocess, sys, build_ext as b\n"
           "sys.exit(subprocess.call(b._compile_cmd(b.ENGINE_SRCS[0], sys.argv[1]) + ['--cuda-host-only']))")


def host_object(tree, obj):
    return subprocess.Popen([sys.executable, "-B", "-c", COMPILE, obj], cwd=os.path.join(tree, "gym-eldorado_amd"),
                            stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def functions(obj):
    text = subprocess.check_output(["objdump", "-d", "-C", "--no-show-raw-insn", obj], text=True)
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+[0-9a-f]+:\s+(.*)$", line)
        if cur is None or not m or re.match(r"^(data16 |cs )*nop|^xchg\s+%ax,%ax", m.group(1)):
            continue
        t = re.sub(r"\b[0-9a-f]+ <([^>+]*)(\+0x[0-9a-f]+)?>", r"<\1>", m.group(1))
        cur.append(re.sub(r"0x[0-9a-f]+\(%rip\)", "X(%rip)", t))
    return {k: v for k, v in out.items() if k.startswith("cog::") and "__device_stub__" not in k}


def main(rev):
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.mkdir(old)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=tar.stdout)
        objs = [os.path.join(tmp, "old.o"), os.path.join(tmp, "new.o")]
        procs = [host_object(old, objs[0]), host_object(ROOT, objs[1])]
        if any(p.wait() for p in procs):
            sys.exit("a compile failed")
        a, b = functions(objs[0]), functions(objs[1])
    print(f"engine host code, {rev} against the working tree: instructions per function")
    print(f"{rev[:8]:>8} {'tree':>6}")
    differs = 0
    for k in sorted(set(a) | set(b)):
        same = a.get(k) == b.get(k)
        differs += not same
        what = "same" if same else "only " + rev[:8] if k not in b else "only tree" if k not in a else "DIFFERS"
        print(f"{len(a.get(k, [])):8d} {len(b.get(k, [])):6d}  {what:13s} {k[:100]}")
    print(f"{differs} of {len(set(a) | set(b))} functions differ or stand on one side only")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) == 2 else sys.exit(__doc__))
