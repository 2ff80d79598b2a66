"""The fixtures of the reader's options (tools/make_golden_opts.py) and the records the
loader's tests build, shared by the CPU and the GPU tests of -q, -B, -Y and -I."""
import gzip
import json
import os

from golden_io import GOLD

MODE_CFY, MODE_IL13 = 0x08, 0x200

with open(os.path.join(GOLD, "manifest_opts.json")) as _f:
    MANIFEST = json.load(_f)
CASES = sorted(k for k, v in MANIFEST.items() if isinstance(v, dict) and "args" in v)


def case_options(name):
    """(mode bits of the reader, trim_qual) of a fixture case's arguments."""
    args = MANIFEST[name]["args"]
    mode = trim = 0
    i = 0
    while i < len(args):
        a = args[i]
        if a == "-q":
            trim = int(args[i + 1])
        elif a == "-B":
            mode |= int(args[i + 1]) << 24
        elif a == "-I":
            mode |= MODE_IL13
        elif a == "-Y":
            mode |= MODE_CFY
        i += 1 if a in ("-I", "-Y") else 2
    return mode, trim


def case_reads(name) -> bytes:
    with gzip.open(os.path.join(GOLD, MANIFEST["files"][MANIFEST[name]["reads"]]), "rb") as f:
        return f.read()


def case_sam(name) -> bytes:
    with gzip.open(os.path.join(GOLD, f"opts_ref_{name}.sam.gz"), "rb") as f:
        return f.read()


def sam_fields(line: bytes):
    """dict of a reference line: name, flag, cigar, seq, qual and the tags by name."""
    f = line.split(b"\t")
    return dict(name=f[0], flag=int(f[1]), cigar=f[5], seq=f[9], qual=f[10], tags={t[:2]: t[5:] for t in f[11:]},
                order=[t[:2] for t in f[11:]])
