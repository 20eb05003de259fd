"""One sorted line per kernel symbol from a build log of the hipcc line in instruct_amd/build.py
(-Rpass-analysis=kernel-resource-usage): demangled name, SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS.

    python -m instruct_amd.build --force 2> build.log
    python tools/kernel_remarks.py build.log > remarks.txt      # diff two of these to compare two commits' device code
"""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]
REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]")


def kernels(log):
    out, cur = {}, None
    for line in log:
        m = REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(path):
    with open(path, errors="replace") as f:
        ks = kernels(f)
    names = demangle(sorted(ks))
    for line in sorted(names[m] + "  " + " ".join(f"{s}={ks[m].get(k, '?')}" for k, s in FIELDS) for m in ks):
        print(line)
    print(f"# {len(ks)} kernel symbols", file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1])
