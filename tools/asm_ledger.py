"""(no GPU) Instruction ledger of one kernel from a disassembly of the built library's gfx950 code object:

    llvm-objcopy --dump-section .hip_fatbin=lib.fatbin instruct_amd/libinstruct_hip.so
    clang-offload-bundler --unbundle --type=o --input=lib.fatbin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=lib.co
    llvm-objdump -d --mcpu=gfx950 lib.co > lib.s
    python tools/asm_ledger.py lib.s 'k_zq_at<256, 5>' [min_valu]

Prints the kernel's instruction count, then every branch-free run of at least `min_valu` (default 150) vector ALU instructions: its
address range, its instructions by issue class and the VALU ones by mnemonic.  The straight-line bodies of a sweep's pass (zq_one) are
such runs; diff the output of two builds to see what a change removed."""
import collections
import re
import subprocess
import sys

HEAD = re.compile(r"^[0-9a-f]+ <(.*)>:\s*$")
INST = re.compile(r"^\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):")


def klass(m):
    if m.startswith(("v_cmp", "v_cmpx")):
        return "valu"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if m.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if m.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc", "s_call")):
        return "branch"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("v_"):
        return "valu"
    return "other"


def main(path, name, min_valu):
    with open(path, errors="replace") as f:
        heads = [h.group(1) for h in (HEAD.match(line) for line in f) if h]
    try:
        plain = subprocess.run(["c++filt"], input="\n".join(heads), capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        plain = heads
    want = {m for m, p in zip(heads, plain) if p.startswith(("void " + name + "(", name + "("))}
    body, inside = [], False
    with open(path, errors="replace") as f:
        for line in f:
            h = HEAD.match(line)
            if h:
                if inside:
                    break
                inside = h.group(1) in want
                continue
            if inside:
                m = INST.match(line)
                if m:
                    body.append((int(m.group(2), 16), m.group(1)))
    if not body:
        sys.exit("kernel not found: " + name)
    tot = collections.Counter(klass(m) for _, m in body)
    print("%s: %d instructions: %s" % (name, len(body), " ".join("%s=%d" % kv for kv in sorted(tot.items()))))
    run = []
    for a, m in body + [(0, "s_endpgm")]:
        if klass(m) == "branch":
            by = collections.Counter(klass(x) for _, x in run)
            if by["valu"] >= min_valu:
                v = collections.Counter(x for _, x in run if klass(x) == "valu")
                print("run %x..%x: %d instructions: %s" % (run[0][0], run[-1][0], len(run), " ".join("%s=%d" % kv for kv in sorted(by.items()))))
                print("   " + " ".join("%s=%d" % kv for kv in sorted(v.items(), key=lambda kv: (-kv[1], kv[0]))))
            run = []
        else:
            run.append((a, m))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 150)
