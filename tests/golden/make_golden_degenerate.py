"""Fixtures for ploidy 4 on degenerate data (tests/degenerate.py; tests/test_degenerate_oracle.py, tests/test_gpu_degenerate.py), written by
the reference's own code.

    python -m instruct_amd.build --oracle && python tests/golden/make_golden_degenerate.py

tg_deg.txt                      the `deg` input: one-allele loci 0 and 69, untyped loci 63 and 64, individuals typed nowhere / at one locus
tg_deg_auto.golden              oracle/_ref/ref_dump_poly (the reference's poly_geno.c sweeps) on it, -ap 1
tg_deg_allo.golden              the same, -ap 0
tg_hom_auto.golden              the `hom` input (no ambiguous genotype), -ap 1; its data file is written to a temporary directory
tg_deg_cli_output.txt           the reference program, -p 4 -ap 1, on tg_deg.txt
tg_deg_allo_cli_output.txt      the reference program, -p 4 -ap 0, on tg_deg.txt
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (also puts the repository on sys.path)
import degenerate as dg  # noqa: E402
from instruct_amd import synth  # noqa: E402

# fixture: (input, allo);  u = 3, b = t = 1, e = 1, r = j = 1, seeds 13 4 1972
CASES = {"tg_deg_auto": ("deg", False), "tg_deg_allo": ("deg", True), "tg_hom_auto": ("hom", False)}
U = 3


def _size(cli, N, L):
    out = list(cli)
    out[out.index("-N") + 1] = str(N)
    out[out.index("-L") + 1] = str(L)
    return out


DEG_CLI = _size(mg.TETRA_CLI, dg.POLY["deg"].N, dg.POLY["deg"].L)
DEG_ALLO_CLI = _size(mg.ALLO_CLI, dg.POLY["deg"].N, dg.POLY["deg"].L)
CLI = {"tg_deg_cli_output.txt": DEG_CLI, "tg_deg_allo_cli_output.txt": DEG_ALLO_CLI}


def dump_args(name, txt, out):
    """the arguments of ref_dump_poly; oracle/orc_dump_poly takes the first 14 the same way"""
    inp, allo = CASES[name]
    p = dg.POLY[inp]
    return [txt, out] + [str(x) for x in (p.K, p.N, p.L, U, 1, 1, 1, 1, 1) + dg.SEEDS] + (["0"] if allo else [])


def main():
    deg_txt = os.path.join(HERE, "tg_deg.txt")
    synth.write_text_polyploid(deg_txt, dg.raw("deg"))
    with tempfile.TemporaryDirectory() as tmp, open(os.devnull, "w") as devnull:
        hom_txt = os.path.join(tmp, "tg_hom.txt")
        synth.write_text_polyploid(hom_txt, dg.raw("hom"))
        for name in sorted(CASES):
            out = os.path.join(HERE, name + ".golden")
            txt = deg_txt if CASES[name][0] == "deg" else hom_txt
            subprocess.check_call([os.path.join(mg.REF, "ref_dump_poly")] + dump_args(name, txt, out), stdout=devnull)
            print(name, os.path.getsize(out), "bytes")
        for fname, cli in CLI.items():
            if os.path.exists(os.path.join(HERE, fname)):
                os.unlink(os.path.join(HERE, fname))
            subprocess.check_call([mg.CLI_REF, "-d", "tg_deg.txt", "-o", fname] + cli, stdout=devnull, cwd=HERE)
            print(fname, os.path.getsize(os.path.join(HERE, fname)), "bytes")


if __name__ == "__main__":
    main()
