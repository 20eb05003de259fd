"""Fixtures for K above 32 (tests/test_oracle_kwide.py, tests/test_gpu_kwide.py), written by the reference's own code.

    python -m instruct_amd.build --oracle && python tests/golden/make_golden_kwide.py

k40.golden               oracle/_ref/ref_dump (the reference's sweeps): N=120, L=200, K=40 on 40-cluster data, 12 iterations; hash
                         lines only (detail 0), and without the N lines of posterior qq means (see trim)
kwide_cli.txt            24 individuals, 60 loci, 40 clusters
k40_cli_output.txt       the reference program at -K 40 on kwide_cli.txt
kscan_32_33_output.txt   the multi-GPU launcher around the reference program: -ik 1 -kv 32 33 on kwide_cli.txt, one worker per K
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (also puts the repository on sys.path)
from instruct_amd import synth  # noqa: E402

# ref_dump arguments after the two paths: K N L u b t c e y r j s1 s2 s3 mode pf detail
K40_DUMP = (40, 120, 200, 12, 4, 4, 1, 1, 1, 2, 2, 13, 4, 1972, 2, 0, 0)
_CLI = ["-L", "60", "-N", "24", "-p", "2", "-u", "40", "-b", "20", "-t", "5", "-v", "2", "-g", "1", "-r", "4", "-j", "4",
        "-lb", "0", "-a", "0", "-s", "13", "4", "1972", "-pi", "0", "-pf", "0"]
K40_CLI = ["-K", "40", "-c", "2"] + _CLI
KSCAN_32_33_CLI = ["-K", "3", "-c", "1"] + _CLI + ["-ik", "1", "-kv", "32", "33"]
MGPU = os.path.join(mg.ROOT, "instruct_amd", "host", "instruct_mgpu")


def k40_dump_data():
    return synth.raw_alleles(120, 200, 40, 2, 2, 0.0, 20261016)


def kwide_cli_data():
    return synth.raw_alleles(24, 60, 40, 2, 2, 0.02, 20261017)


def dump_args(txt, out):
    return [txt, out] + [str(x) for x in K40_DUMP]


def trim(data):
    """a trajectory file without its `chain qq` lines (N lines of 2 K posterior means each: most of the file at K = 40)"""
    return b"".join(l for l in data.splitlines(True) if not l.startswith(b"chain qq "))


def main():
    txt = os.path.join("/tmp", "k40.txt")
    synth.write_text_diploid(txt, k40_dump_data())
    with open(os.devnull, "w") as devnull:
        subprocess.check_call([os.path.join(mg.REF, "ref_dump")] + dump_args(txt, "/tmp/k40.golden"), stdout=devnull)
    with open("/tmp/k40.golden", "rb") as f, open(os.path.join(HERE, "k40.golden"), "wb") as g:
        g.write(trim(f.read()))
    synth.write_text_diploid(os.path.join(HERE, "kwide_cli.txt"), kwide_cli_data())
    with open(os.devnull, "w") as devnull:
        subprocess.check_call([mg.CLI_REF, "-d", "kwide_cli.txt", "-o", "k40_cli_output.txt"] + K40_CLI, stdout=devnull, cwd=HERE)
        subprocess.check_call([os.path.relpath(MGPU, HERE), "--exe", mg.CLI_REF, "--gpus", "1", "--", "-d", "kwide_cli.txt", "-o", "kscan_32_33_output.txt"]
                              + KSCAN_32_33_CLI, stdout=devnull, cwd=HERE)
    for name in ("k40.golden", "kwide_cli.txt", "k40_cli_output.txt", "kscan_32_33_output.txt"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
