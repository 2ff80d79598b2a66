"""The sequential restatement of the hit choice (tests/choose_ref.py) against glibc, and
hsa_amd.sam.sam_line against lines the reference program printed."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import choose_ref as cr
from golden_io import GOLD
from hsa_amd import sam


def erand48_draws(state, n):
    libc = C.CDLL("libc.so.6")
    libc.erand48.restype = C.c_double
    xs = (C.c_ushort * 3)(state & 0xFFFF, (state >> 16) & 0xFFFF, (state >> 32) & 0xFFFF)
    return [libc.erand48(xs) for _ in range(n)], xs[0] | (xs[1] << 16) | (xs[2] << 32)


@pytest.mark.parametrize("state", [cr.SEED0, 0x1234ABCD330E, (1 << 48) - 1, 0x5A5A12345678])
def test_generator_is_glibc_erand48(state):
    want, end = erand48_draws(state, 10000)
    x, got = state, []
    for _ in range(10000):
        x = cr.step(x)
        got.append(cr.real(x))
    assert got == want and x == end


def test_default_state_is_the_unseeded_process_s():
    """drand48 in a fresh process that never seeds, as the reference program is: glibc starts
    from X = 0 (not from the 0x1234ABCD330E of the SVID text: only srand48 puts 0x330E in the
    low word)."""
    import subprocess
    import sys
    code = "import ctypes as C; L = C.CDLL('libc.so.6'); L.drand48.restype = C.c_double; print([L.drand48().hex() for _ in range(4)])"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    x, want = cr.SEED0, []
    for _ in range(4):
        x = cr.step(x)
        want.append(cr.real(x).hex())
    assert out.strip() == str(want)
    from hsa_amd._lib import DRAND48_SEED0
    assert DRAND48_SEED0 == cr.SEED0


@pytest.mark.parametrize("d", [0, 1, 2, 63, 64, 65, (1 << 20) + 3])
def test_jump_is_d_steps(d):
    for state in (cr.SEED0, 0x1234ABCD330E, 0xFFFFFFFFFFFF):
        x = state
        for _ in range(d):
            x = cr.step(x)
        assert cr.jump(state, d) == x


def test_zero_predecessor_and_log_table():
    assert cr.real(cr.step(cr.zero_predecessor())) == 0.0
    from hsa_amd._lib import log_n_table
    t = log_n_table()
    assert np.array_equal(t, cr.log_n_table()) and t[1] == 0 and t[2] == 3 and t[255] == 24


# ---------------------------------------------------------------- sam_line
OPS = {c: i for i, c in enumerate("MIDNS")}


def rows_of_line(line, chr_names):
    """The device's outputs for a reference line, made by hand from the line's own fields:
    what choose_hits64 and refine_rows64 would hold for it."""
    f = line.split("\t")
    tags = {x[:2]: x[5:] for x in f[11:]}
    strand = (int(f[1]) >> 4) & 1
    lut = {c: i for i, c in enumerate("ACGTN")}
    seq = np.array([lut[c] for c in f[9]], np.uint8)
    if strand:
        seq = np.array([{0: 3, 1: 2, 2: 1, 3: 0, 4: 4}[int(c)] for c in seq[::-1]], np.uint8)
    qual = f[10][::-1] if strand else f[10]
    entries = [(f[2], strand, int(f[3]), f[5], int(tags["XM"]), int(tags["XO"]), int(tags["XG"]), tags["MD"], int(tags["NM"]))]
    # an XA entry is "<chr>,<sign><pos>,<diffs>;" or "<chr>,<sign><pos><CIGAR>": the position's
    # digits run into the CIGAR's, and the split is where the CIGAR spans the read
    for m in re.finditer(r"([^,;]+?),([+-])([\dMIDS]+)(,\d+;)?", tags.get("XA", "")):
        run, gapped = m.group(3), m.group(4) is None
        if gapped:
            cut = next(i for i in range(1, len(run)) if re.fullmatch(r"(\d+[MIDS])+", run[i:]) and run[i] != "0" and
                       sum(int(k) for k, c in re.findall(r"(\d+)([MIDS])", run[i:]) if c != "D") == len(seq))
            run, cg = run[:cut], run[cut:]
        entries.append((m.group(1), int(m.group(2) == "-"), int(run), cg if gapped else f"{len(seq)}M",
                        0 if gapped else int(m.group(4)[1:-1]), int(gapped), int(gapped), "", 0))
    n = len(entries)
    rows, rpos, pos = np.zeros((n, 8), np.uint32), np.zeros((n, 2), np.uint64), np.zeros((n, 4), np.uint64)
    cigar, md, hits = np.zeros((n, 8), np.uint32), np.zeros((n, 64), np.uint8), np.zeros((n, 14), np.uint32)
    for t, (ch, st, p, cg, xm, xo, xg, mds, nm) in enumerate(entries):
        ops = re.findall(r"(\d+)([MIDS])", cg)
        cigar[t, :len(ops)] = [(OPS[c] << 28) | int(k) for k, c in ops]
        md[t, :len(mds)] = np.frombuffer(mds.encode(), np.uint8)
        rows[t, :4] = (0, len(ops), nm, len(mds))
        rpos[t] = (p - 1, p)
        pos[t] = (p - 1, chr_names.index(ch), p, p - 1)
        hits[t, 0] = xm | (xo << 16) | ((xg - xo) << 24)
        hits[t, 1] = st << 30
    typ = "NUR".index(tags["XT"])
    sel = np.array([typ, 0, int(f[4]), n - 1], np.uint32)
    sel64 = np.array([0, int(tags["X0"]), int(tags.get("X1", 0)), 0], np.uint64)
    return dict(name=f[0], seq_codes=seq, qual=qual, chr_names=chr_names, sel=sel, sel64=sel64, rows=rows, rpos=rpos,
                cigar=cigar, md=md, pos=pos, hits=hits)


def rep_lines():
    with open(os.path.join(GOLD, "choose_ref_lines.sam")) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip() and ln[0] != "@"]


def test_unique_line_of_the_dropin_fixture():
    lines = [ln for ln in gzip.open(os.path.join(GOLD, "dropin_ref_default.sam.gz"), "rt").read().split("\n")
             if "XT:A:U" in ln]
    names = ["chr1", "chr2", "chr3"]
    gapped = next(ln for ln in lines if re.search(r"\t\d+M\d+[ID]\d+M\t", ln) and ln.split("\t")[1] == "16")
    for ln in (lines[0], gapped):
        assert sam.sam_line(**rows_of_line(ln, names), max_top2=30) == ln


def test_repeat_and_xa_lines_of_the_reference_program():
    """Lines `HSA aln -n 4 -o 1` (and `-R 1` for the first) printed for reads of the repeat
    genome: XT:A:R with X1 absent because X0 > max_top2; XA entries of both forms."""
    lines = rep_lines()
    no_x1 = [ln for ln in lines if "XT:A:R" in ln and "X1:i" not in ln]
    assert len(no_x1) >= 2
    for ln in lines:
        x0 = int(re.search(r"X0:i:(\d+)", ln).group(1))
        top2 = 30 if ("X1:i" in ln) == (x0 <= 30) else 1         # the -R 1 run's lines
        assert sam.sam_line(**rows_of_line(ln, ["chr1"]), max_top2=top2) == ln
    assert any(re.search(r"XA:Z:\S*\d+[MID]", ln) for ln in lines) and any(re.search(r"XA:Z:\S*,\d+;", ln) for ln in lines)


def test_xa_list_with_a_gapped_and_an_ungapped_entry():
    """No line of the reference's SAM on the repeat genome holds both forms in one list
    (4 000 reads searched), so this one is put together from two of its lines: the quirk of
    bwtse.c:789-795 is per entry, a gapped one printing its CIGAR and no ';'."""
    lines = rep_lines()
    g = next(ln for ln in lines if "X1:i" in ln and re.search(r"XA:Z:[^,]+,[+-]\d+M\d+[ID]\d+M$", ln))
    u = next(ln for ln in lines if re.search(r"XA:Z:[^,]+,[+-]\d+,\d+;$", ln))
    a, b = rows_of_line(g, ["chr1"]), rows_of_line(u, ["chr1"])
    for k in ("rows", "rpos", "cigar", "md", "pos", "hits"):
        a[k] = np.concatenate([a[k], b[k][1:]])
    a["sel"][3] = 2
    assert sam.sam_line(**a, max_top2=30) == g + u.split("XA:Z:")[1]
    with pytest.raises(ValueError):
        sam.sam_line(**dict(a, sel=np.array([0, 0, 0, 0], np.uint32)))
