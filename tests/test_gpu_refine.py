"""Position rows of the 64-bit path refined into CIGAR, NM and MD on the device
(hsa_refine_rows_device64, hsa_index_set_text64_device).

* against the compiled reference's SAM: the committed drop-in fixtures (every XT:A:U / R
  line of `HSA aln` with defaults and with -n 4 -o 0), and the reference program run here
  on a repeat genome and on 250 bp reads;
* past 2^32, where no reference exists: validity of every answered row against the text,
  exactness by translating each row's window into a small text (whose side the SAM tests
  pin to the reference), and the text's end;
* the contract's edges on small fabricated batches;
* against the compiled reference's own bwa_refine_gapped on fabricated rows: the committed
  fixture tests/golden/refine_cases.npz (tests/refine_cases.py: ties inside repeats, long
  deletions across the band's 64-column chunks, indels at the ends, N, odd lengths, windows
  cut by the text's end, every text alignment), field for field, in three batch layouts,
  and a fresh random set where the reference's driver is built."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from golden_io import GOLD, INDEX, parse_opts
from hsa_amd import index_io
from hsa_amd.chain import to_device as dev
from hsa_amd.reads import cal_maxdiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSA = os.path.join(ROOT, "oracle", "_ref", "HSA")
REF_REFINE = os.path.join(ROOT, "oracle", "_ref", "ref_refine")
MAN = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
U64 = np.uint64
ONES = U64(0xFFFFFFFFFFFFFFFF)
BIG_T = (1 << 32) + (1 << 22) + 7
SEED_NONE = 0x7FFFFFFF
_IX = {}


def tiny_like(name, text=True):
    """A fresh hsa_index_create_device64 handle over a golden index: both suffix arrays
    and, with `text`, the .pac text through set_text (the host's MSB-first words)."""
    from hsa_amd._lib import GpuIndex
    from test_gpu_sa64 import widen
    from test_gpu_wide import _upload_lsb
    fwd, rev = index_io.read_index(INDEX[name])
    d_f, d_r = _upload_lsb(fwd), _upload_lsb(rev)
    gi = GpuIndex.from_device_codes64(fwd.T, fwd.isa0, np.asarray(fwd.C, U64), d_f.data_ptr(), rev.T, rev.isa0,
                                      np.asarray(rev.C, U64), d_r.data_ptr())
    sa, blocks = index_io.read_sa(INDEX[name]), index_io.read_blocks(INDEX[name])
    gi.set_sa(sa, blocks)
    gi.set_sa64(widen(sa.values), sa.interval, blocks.astype(U64))
    if text:
        gi.set_text(*index_io.read_packed_dna(INDEX[name]))
    return gi


def index_text(name):
    if name not in _IX:
        _IX[name] = tiny_like(name)
    return _IX[name]


def search_rows(gi, lens, codes, od, max_occ, cap_per_read=64):
    """hsa_search_device64 then hsa_hit_positions_device64 of one batch, everything left
    on the device: (device tensors for the refinement, host copies)."""
    from hsa_amd import chain
    from hsa_amd._lib import ALN64_WORDS, pad_codes, regime_of
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    md = np.array([cal_maxdiff(int(l), thres=od["fnr"]) for l in lens], np.int32) if od["fnr"] > 0 else od["max_diff"]
    loc, n_stacks, _ = chain.local_regime(od, int(lens.max()))
    jobs = chain.make_jobs(lens, md, od["seed_len"])
    b = dict(jobs=dev(jobs), codes=dev(pad_codes(codes)), n_jobs=n, max_len=int(lens.max()))
    cap = n * cap_per_read
    t = chain.search64(gi, b, 0, n, regime_of(od, n_stacks, loc["max_diff"]), od["seed_len"], hit_cap=cap)
    assert int(t["sc"][11]) == 0 and t["hit_cap"] == cap, "reads left unfinished"
    t = dict(b, **chain.hit_positions64(gi, t, n, max_occ, fill=0x77))
    host = dict(flags=t["flags"].cpu().numpy().astype(np.uint32), hit_off=t["hit_off"].cpu().numpy(),
                hits=t["hits"].cpu().numpy().view(np.uint32)[:cap * ALN64_WORDS].reshape(-1, ALN64_WORDS),
                pos_off=t["pos_off"].cpu().numpy(), pos=t["pos"].cpu().numpy().view(U64).reshape(-1, 4),
                pos_hit=t["pos_hit"].cpu().numpy().view(np.uint32), lens=lens, codes=np.asarray(codes, np.uint8),
                offs=jobs["off"].astype(np.int64))
    return t, host


def fabricate(lens, codes, rows):
    """A batch made by hand: rows = (read, strand, gap, text position, in-chromosome
    position), in read order; one hit record per row."""
    import torch
    from hsa_amd.chain import make_jobs
    from hsa_amd._lib import ALN64_WORDS, pad_codes
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    jobs = make_jobs(lens, 0, 0)
    reads = np.array([r[0] for r in rows], np.int64)
    assert (np.diff(reads) >= 0).all()
    cnt = np.bincount(reads, minlength=n)[:n]
    pos_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    hits = np.zeros((max(len(rows), 1), ALN64_WORDS), np.uint32)
    pos = np.zeros((max(len(rows), 1), 4), U64)
    for k, (_, strand, gap, p, ori) in enumerate(rows):
        go = 1 if gap else 0
        hits[k, 0] = (go << 16) | ((gap - go) << 24)
        hits[k, 1] = strand << 30
        pos[k] = (p, 1, ori, p)
    pos_hit = (np.arange(len(rows)) - pos_off[reads]).astype(np.uint32) if len(rows) else np.zeros(1, np.uint32)
    t = dict(jobs=dev(jobs), codes=dev(pad_codes(codes)), hit_off=dev(pos_off[:-1]),
             hits=dev(hits), pos_off=dev(pos_off), pos=dev(pos), pos_hit=dev(pos_hit),
             pos_ctr=dev(np.array([len(rows), len(rows), 0, 0], np.int64)), n_jobs=n, max_len=int(lens.max()),
             pos_cap=len(rows))
    torch.cuda.synchronize()
    host = dict(hit_off=pos_off[:-1], hits=hits, pos_off=pos_off, pos=pos, pos_hit=pos_hit, lens=lens,
                codes=np.asarray(codes, np.uint8), offs=jobs["off"].astype(np.int64))
    return t, host


def refine(gi, t, cigar_stride=8, md_stride=64, guard=0, counters=True, pos_cap=None):
    """One hsa_refine_rows_device64 call: (rows (n, 8), rpos (n, 2), cigar (n, cs), md (n,
    ms), counters) as NumPy arrays, `guard` filled rows kept past pos_cap."""
    import torch
    from hsa_amd._lib import RF_ROW_WORDS, RefineBatch64
    cap = t["pos_cap"] if pos_cap is None else pos_cap
    m = max(cap + guard, 1)
    o = dict(rows=torch.full((m * RF_ROW_WORDS,), 0x77, dtype=torch.int32, device="cuda"),
             rpos=torch.full((m * 2,), 0x77, dtype=torch.int64, device="cuda"),
             cigar=torch.full((max(m * cigar_stride, 1),), 0x77, dtype=torch.int32, device="cuda"),
             md=torch.full((max(m * md_stride, 1),), 0x77, dtype=torch.uint8, device="cuda"),
             ctr=torch.full((8,), 0x33, dtype=torch.int64, device="cuda"))
    b = RefineBatch64(d_jobs=t["jobs"].data_ptr(), n_jobs=t["n_jobs"], d_codes=t["codes"].data_ptr(),
                      d_hit_off=t["hit_off"].data_ptr(), d_hits=t["hits"].data_ptr(), d_pos_off=t["pos_off"].data_ptr(),
                      d_pos=t["pos"].data_ptr(), d_pos_hit=t["pos_hit"].data_ptr(), pos_cap=cap,
                      d_pos_counters=t["pos_ctr"].data_ptr() if counters else None, max_len=t["max_len"],
                      cigar_stride=cigar_stride, md_stride=md_stride, d_rows=o["rows"].data_ptr(),
                      d_rpos=o["rpos"].data_ptr(), d_cigar=o["cigar"].data_ptr(), d_md=o["md"].data_ptr(),
                      d_counters=o["ctr"].data_ptr())
    torch.cuda.synchronize()
    gi.refine_rows64(b)
    torch.cuda.synchronize()
    return dict(rows=o["rows"].cpu().numpy().view(np.uint32).reshape(m, RF_ROW_WORDS),
                rpos=o["rpos"].cpu().numpy().view(U64).reshape(m, 2),
                cigar=o["cigar"].cpu().numpy().view(np.uint32)[:m * cigar_stride].reshape(m, cigar_stride),
                md=o["md"].cpu().numpy()[:m * md_stride].reshape(m, md_stride), ctr=o["ctr"].cpu().numpy().view(U64))


def same(a, b, n=None):
    return all(np.array_equal(a[k][:n], b[k][:n]) for k in ("rows", "rpos", "cigar", "md")) and \
        np.array_equal(a["ctr"][:7], b["ctr"][:7])


def row_strings(out, t):
    from hsa_amd import refine as rf
    return rf.row_sam(out["rows"][t], out["cigar"][t], out["md"][t])


def oriented(host, r, strand):
    """The read as the SAM stage hands it to the alignment: strand ? rseq : seq."""
    from hsa_amd import synth
    sq = host["codes"][host["offs"][r]:host["offs"][r] + int(host["lens"][r])]
    return synth.revcomp_codes(sq) if strand else sq


def replay(out, t, seq, text_at):
    """A row is *valid*: its CIGAR spans the read, NM is the M columns' mismatches plus the
    I and D lengths, and its MD spells the text at the refined position."""
    rs = row_strings(out, t)
    ops = [(int(n), c) for n, c in re.findall(r"(\d+)([MIDS])", rs["cigar"])]
    assert "".join(f"{n}{c}" for n, c in ops) == rs["cigar"] and ops
    x, y, nm, md, u = int(out["rpos"][t, 0]), 0, 0, "", 0
    for n, c in ops:
        if c == "M":
            ref = text_at(np.arange(x, x + n))
            for z in range(n):
                if seq[y + z] > 3 or ref[z] != seq[y + z]:
                    md += f"{u}{'ACGT'[ref[z]]}"
                    nm += 1
                    u = 0
                else:
                    u += 1
            x += n
            y += n
        elif c in "IS":
            y += n
            nm += n if c == "I" else 0
        else:
            md += f"{u}^" + "".join("ACGT"[b] for b in text_at(np.arange(x, x + n)))
            u = 0
            x += n
            nm += n
    md += str(u)
    assert y == len(seq), f"row {t}: the CIGAR {rs['cigar']} spans {y} of {len(seq)} read bases"
    assert nm == rs["nm"], f"row {t}: NM {rs['nm']}, the replay counts {nm} ({rs['cigar']})"
    assert md == rs["md"], f"row {t}: MD {rs['md']}, the text spells {md}"


# ---------------------------------------------------------------- against the reference's SAM
def sam_lines(raw):
    out = []
    for ln in raw.decode().splitlines():
        if not ln or ln[0] == "@":
            continue
        f = ln.split("\t")
        tags = {x[:2]: x[5:] for x in f[11:]}
        out.append(dict(name=f[0], strand=(int(f[1]) >> 4) & 1, chr=f[2], pos=int(f[3]), cigar=f[5], tags=tags,
                        unmapped=bool(int(f[1]) & 4)))
    return out


def chrom_starts(name):
    """chromosome name -> (text position of its first base, ori of its block): the golden
    indexes have one block per chromosome."""
    with open(INDEX[name] + ".index.ann") as f:
        ls = f.read().split("\n")
    n_chr = int(ls[0].split()[1])
    names = [ls[1 + k].split()[1] for k in range(n_chr)]
    blocks = index_io.read_blocks(INDEX[name])
    assert len(blocks) == n_chr
    return {names[int(b[0])]: (int(b[1]), int(b[3])) for b in blocks}


def fastq_codes(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        ls = f.read().split("\n")
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = lut[ord(c.lower())] = i
    names = [ls[k][1:].split()[0] for k in range(0, len(ls) - 3, 4)]
    seqs = [lut[np.frombuffer(ls[k + 1].encode(), np.uint8)] for k in range(0, len(ls) - 3, 4)]
    return names, seqs


def searched(seqs, od):
    """The reads bwa_cal_sa_reg_gap searches (bwtaln.c:314-325): not the ones with more N
    than differences, nor the poly-A / poly-T ones."""
    keep = []
    for r, sq in enumerate(seqs):
        md = cal_maxdiff(len(sq), thres=od["fnr"]) if od["fnr"] > 0 else od["max_diff"]
        polyat = len(sq) >= 15 and ((sq[:15] == 0).all() or (sq[:15] == 3).all())
        if int((sq > 3).sum()) <= md and not polyat:
            keep.append(r)
    return keep


def check_lines(gi, index, names, seqs, lines, args, max_occ):
    """Every XT:A:U / XT:A:R line has a row of its read with the line's strand, chromosome,
    POS, CIGAR, NM and MD.  The reads are searched as the drop-in searches them: the
    caller's options with gap extensions counted as differences (bwtaln.c:261) up to and
    including the first read without a hit, the batch's local options after it.
    A read the search leaves without a hit on either strand (HSA_F_FALLBACK) has no rows: if
    the reference prints a U / R line for it, the line comes from the host's splice path
    (bwt_splice_match returning an unspliced alignment), which has no 64-bit counterpart;
    such lines are returned apart, not checked."""
    from oracle_ctypes import default_opt
    base = parse_opts(args, default_opt())
    keep = searched(seqs, base)
    lens = np.array([len(seqs[r]) for r in keep], np.uint32)
    codes = np.concatenate([seqs[r] for r in keep])
    job_of = {names[r]: j for j, r in enumerate(keep)}
    od_a = dict(base)
    od_a["mode"] &= ~0x01
    t, host = search_rows(gi, lens, codes, od_a, max_occ)
    runs = [(host, refine(gi, t, cigar_stride=16, md_stride=128))]
    fb = np.flatnonzero(host["flags"] & 1)
    switch = int(fb[0]) if len(fb) else len(lens)           # the first read without a hit
    if switch < len(lens) - 1:
        t, host = search_rows(gi, lens, codes, base, max_occ)
        runs.append((host, refine(gi, t, cigar_stride=16, md_stride=128)))
    starts = chrom_starts(index)
    todo = [ln for ln in lines if ln["tags"].get("XT") in ("U", "R")]
    missing, no_hit = [], []
    for ln in todo:
        j = job_of[ln["name"]]
        host, out = runs[0] if j <= switch or len(runs) == 1 else runs[1]
        if host["flags"][j] & 1:
            no_hit.append(ln["name"])
            continue
        first, ori = starts[ln["chr"]]
        want_pos = first + ln["pos"] - 1 - ori
        hit = False
        for row in range(int(host["pos_off"][j]), int(host["pos_off"][j + 1])):
            rec = host["hits"][int(host["hit_off"][j]) + int(host["pos_hit"][row])]
            if int(rec[1] >> 30) != ln["strand"] or int(out["rpos"][row, 0]) != want_pos or int(out["rpos"][row, 1]) != ln["pos"]:
                continue
            if int(out["rows"][row, 0]) != 0:
                continue
            rs = row_strings(out, row)
            if rs["cigar"] == ln["cigar"] and rs["nm"] == int(ln["tags"]["NM"]) and rs["md"] == ln["tags"]["MD"]:
                hit = True
                break
        if not hit:
            missing.append(ln["name"])
    assert not missing, f"{len(missing)} of {len(todo)} lines have no matching row, first {missing[:5]}"
    return todo, runs, no_hit


@pytest.mark.parametrize("name", ["default", "n4o0"])
def test_golden_sam_lines_have_their_rows(name):
    gi = index_text("tiny")
    names, seqs = fastq_codes(os.path.join(GOLD, MAN["reads"]))
    lines = sam_lines(gzip.open(os.path.join(GOLD, f"dropin_ref_{name}.sam.gz")).read())
    todo, runs, no_hit = check_lines(gi, "tiny", names, seqs, lines, MAN[name]["args"], 64)
    assert not no_hit, f"lines of reads the search gives no hit: {no_hit[:5]}"      # no line may be left out
    if name == "default":       # what the fixture holds: gapped lines on both strands, ^ runs, an I with a D
        assert len(todo) == 890 and sum(("I" in ln["cigar"] or "D" in ln["cigar"]) for ln in todo) == 365
        assert sum("^" in ln["tags"]["MD"] for ln in todo) == 183
        assert int(runs[0][1]["ctr"][6]) >= 365                  # rows that ran the alignment
    else:
        assert len(todo) == 526 and int(runs[0][1]["ctr"][6]) == 0   # ungapped: the MD-only kernel


@pytest.mark.skipif(not os.path.exists(HSA), reason="oracle/_ref/HSA not built (make -C oracle)")
@pytest.mark.parametrize("index,n,L,mmi", [("rep", 300, 60, 1), ("tiny", 20, 250, 1)])
def test_reference_program_lines_have_their_rows(tmp_path, index, n, L, mmi):
    """Multi-hit reads (the repeat genome) and long reads: the primary line of every
    XT:A:U / R read of the reference program's own SAM, -n 4 -o 1, that the main search gives
    a hit (check_lines: the others' lines come from the host's splice path)."""
    from hsa_amd import synth
    text = index_io.read_pac(INDEX[index])
    reads, _ = synth.make_reads(text, [(0, len(text))], n, L, 733, indel=True, max_mm_indel=mmi)
    fq = str(tmp_path / "reads.fq")
    synth.write_fastq(fq, reads)
    args = ["-n", "4", "-o", "1"]
    r = subprocess.run([HSA, "aln", *args, INDEX[index], fq], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = sam_lines(r.stdout)
    ur = [ln for ln in lines if ln["tags"].get("XT") in ("U", "R")]
    most = max(int(ln["tags"]["X0"]) + int(ln["tags"].get("X1", 0)) for ln in ur)
    max_occ = 64 if index == "tiny" else 256
    assert most <= max_occ, f"X0 + X1 = {most}: the reference alone would leave lines out at max_occ {max_occ}"
    names, seqs = fastq_codes(fq)
    todo, _, no_hit = check_lines(index_text(index), index, names, seqs, lines, args, max_occ)
    # (the repeat genome's set: 4 of 242 lines are of reads without a main-search hit, printed from the splice path)
    assert len(todo) > n // 2 and len(no_hit) <= len(todo) // 20, (len(todo), no_hit)
    if index == "rep":
        assert any(ln["tags"]["XT"] == "R" for ln in todo)


# ---------------------------------------------------------------- contract edges
def tiny_batch():
    """Rows on the tiny text by hand: reads cut from it with a substitution or an indel."""
    text = index_io.read_pac(INDEX["tiny"])
    from hsa_amd import synth
    a = text[1000:1100].copy()
    a[17] ^= 1
    a[18] ^= 2                                   # two adjacent mismatches: a zero-length count in MD
    b = np.concatenate([text[5000:5040], text[5043:5103]])              # a 3 bp deletion
    c = synth.revcomp_codes(np.concatenate([text[9000:9050], [0, 1], text[9050:9098]]).astype(np.uint8))  # reverse, 2 bp insertion
    lens = [100, 100, 100]
    codes = np.concatenate([a, b, c]).astype(np.uint8)
    rows = [(0, 0, 0, 1000, 1001), (1, 0, 3, 5000, 5001), (2, 1, 2, 9000, 9001)]
    return lens, codes, rows, text


def test_fabricated_rows_status_strides_and_guards():
    from hsa_amd import _lib
    gi = index_text("tiny")
    lens, codes, rows, text = tiny_batch()
    rows = rows[:1] + [(0, 0, 0, int(ONES), int(ONES))] + rows[1:]     # an all-ones position row
    t, host = fabricate(lens, codes, rows)
    out = refine(gi, t, guard=16)
    n = len(rows)
    assert [int(s) for s in out["rows"][:n, 0]] == [0, _lib.HSA_RF_POS, 0, 0]
    assert [int(x) for x in out["ctr"][:7]] == [n, 3, 1, 0, 0, 0, 2]
    assert row_strings(out, 0) == dict(status=0, cigar="100M", nm=2, trim5=0, trim3=0,
                                       md=f"17{'ACGT'[text[1017]]}0{'ACGT'[text[1018]]}81")
    # (where exactly the alignment puts an indel among equal bases is the reference's tie rule: the SAM tests pin it)
    assert re.fullmatch(r"\d+M3D\d+M", row_strings(out, 2)["cigar"]) and row_strings(out, 2)["nm"] == 3
    assert re.fullmatch(r"\d+M2I\d+M", row_strings(out, 3)["cigar"]) and row_strings(out, 3)["nm"] == 2
    for k, strand in ((0, 0), (2, 0), (3, 1)):
        replay(out, k, oriented(host, rows[k][0], strand), lambda p: text[p])
    assert int(out["rpos"][2, 0]) == 5000 and int(out["rpos"][2, 1]) == 5001
    # guard rows after the last row are untouched
    assert (out["rows"][n:] == 0x77).all() and (out["rpos"][n:] == U64(0x77)).all()      # (refine()'s fill)
    assert (out["cigar"][n:] == 0x77).all() and (out["md"][n:] == 0x77).all()
    # two runs give equal arrays; without the position call's counters the count is pos_off's
    assert same(out, refine(gi, t, guard=16))
    assert same(out, refine(gi, t, guard=16, counters=False))
    # an MD stride one byte short: HSA_RF_MD with the needed length; enlarged, OK
    need = int(out["rows"][2, 3])
    short = refine(gi, t, md_stride=need - 1)
    assert int(short["rows"][2, 0]) == _lib.HSA_RF_MD and int(short["rows"][2, 3]) == need
    assert np.array_equal(short["md"][2], out["md"][2, :need - 1])
    exact = refine(gi, t, md_stride=need)
    assert int(exact["rows"][2, 0]) == 0 and np.array_equal(exact["md"][2], out["md"][2, :need])
    one = refine(gi, t, cigar_stride=2)                                # and a CIGAR stride one op short
    assert int(one["rows"][2, 0]) == _lib.HSA_RF_MD and int(one["rows"][2, 1]) == 3
    assert int(one["rows"][0, 0]) == 0
    # a clone shares the text
    c = gi.clone()
    assert same(out, refine(c, t, guard=16))
    c.close()


def test_no_rows_return_cleanly():
    from hsa_amd._lib import RefineBatch64
    import torch
    gi = index_text("tiny")
    ctr = torch.full((8,), 0x33, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gi.refine_rows64(RefineBatch64(n_jobs=0, d_counters=ctr.data_ptr()))          # no jobs at all
    torch.cuda.synchronize()
    assert not ctr.cpu().numpy().any()
    lens, codes, _, _ = tiny_batch()
    t, _ = fabricate(lens, codes, [])                                             # reads without a row
    for counters in (True, False):
        out = refine(gi, t, guard=4, counters=counters, pos_cap=3)
        assert not out["ctr"][:7].any() and (out["rows"] == 0x77).all()


def test_longest_read_and_widest_gap_of_the_layout_are_answered(golden_side):
    """len 1023 with a gap count of 16, a deletion and an insertion on both strands: answered
    with the reference's own strings (the fixture's `longest` rows), and valid."""
    from hsa_amd import _lib
    gi, text = golden_side
    long = [r for r in rc.golden()[2] if r["family"].startswith("longest")]
    assert sorted((r["strand"], "16D" in r["made"], r["len"], r["gap"]) for r in long) == \
        [(0, False, 1023, 16), (0, True, 1023, 16), (1, False, 1023, 16), (1, True, 1023, 16)]
    t, host = golden_batch(long)
    out = refine(gi, t, cigar_stride=16, md_stride=256)
    assert [int(s) for s in out["rows"][:, 0]] == [0] * 4 and int(out["ctr"][6]) == 4 and int(out["ctr"][4]) == 0
    for k, r in enumerate(long):
        rs = row_strings(out, k)
        assert (rs["cigar"], rs["nm"], rs["md"]) == (r["cigar"], r["nm"], r["md"]), (r["made"], rs, r["cigar"], r["md"])
        replay(out, k, oriented(host, k, r["strand"]), lambda p: text[p])
    assert any("16D" in r["cigar"] for r in long) and any("16I" in r["cigar"] for r in long)
    # past the layout: a gap count of HSA_RF_MAX_GAP + 1 is refused, not approximated
    r = long[0]
    t2, _ = fabricate([1023], r["codes"], [(0, r["strand"], _lib.HSA_RF_MAX_GAP + 1, r["pos"], r["ori"])])
    assert int(refine(gi, t2)["rows"][0, 0]) == _lib.HSA_RF_CAP


def test_set_text64_device_rules_and_layouts_agree():
    """Refused on a clone, on a 32-bit-only handle and with a T that is not the index's (the
    array stays the caller's); attached, the LSB-first text answers as the host's packed
    text does."""
    from hsa_amd._lib import DeviceU64, GpuIndex, HsaError
    text = index_io.read_pac(INDEX["tiny"])
    T = len(text)
    w = index_io.pack_lsb_u32(text)
    w = np.concatenate([w, np.zeros(len(w) % 2 + 2, np.uint32)])
    d = DeviceU64(len(w) // 2)
    d.write(0, w.view(U64))
    gi = tiny_like("tiny", text=False)
    lens, codes, rows, _ = tiny_batch()
    t, _ = fabricate(lens, codes, rows)
    with pytest.raises(HsaError, match="-2"):                        # no text yet
        refine(gi, t)
    with pytest.raises(HsaError, match="-2"):                        # T not the index's
        gi.set_text64_device(d.ptr, T - 1)
    c = gi.clone()
    with pytest.raises(HsaError, match="-2"):                        # a clone
        c.set_text64_device(d.ptr, T)
    with pytest.raises(HsaError, match="-2"):                        # an index with live clones
        gi.set_text64_device(d.ptr, T)
    c.close()
    narrow = GpuIndex(*index_io.read_index(INDEX["tiny"]))           # not an index of hsa_index_create_device64
    with pytest.raises(HsaError, match="-2"):
        narrow.set_text64_device(d.ptr, T)
    narrow.close()
    assert np.array_equal(d.to_host(0, 4), w.view(U64)[:4])          # still the caller's, still whole
    gi.set_text64_device(d, T)
    assert d.ptr is None
    got = refine(gi, t)
    assert same(got, refine(index_text("tiny"), t))
    c = gi.clone()                                                   # a clone shares it
    assert same(got, refine(c, t))
    c.close()
    gi.close()


# ---------------------------------------------------------------- past 2^32
@pytest.fixture(scope="module")
def big_text64():
    """The 4.3 Gbp synthetic text of test_gpu_sa64's big64 (seed 77) with its text kept on
    the device and attached: 2^32 + 2^22 + 7 characters is the smallest text that has the
    edge at all."""
    import torch
    from hsa_amd import synth
    from hsa_amd._lib import DeviceU64, GpuIndex, HsaError, build_bwt_index64, check, lib
    T = BIG_T
    nw = (T + 15) // 16
    text = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    check(lib().hsa_synth_genome_device(0, T, 77, text.data_ptr()))
    torch.cuda.synchronize()
    bw, isa0, Cf, sa = build_bwt_index64(T, text.data_ptr(), 32)
    rb = torch.zeros(nw + 8, dtype=torch.int32, device="cuda")
    i0 = C.c_uint64()
    Cr = np.zeros(5, U64)
    check(lib().hsa_build_bwt_device64(0, T, text.data_ptr(), 1, rb.data_ptr(), C.byref(i0), Cr))
    d_text = DeviceU64((nw + 2) // 2)
    rc = lib().hipMemcpy(C.c_void_p(d_text.ptr), C.c_void_p(text.data_ptr()), C.c_size_t(4 * nw), 3)
    if rc != 0:
        raise HsaError(f"hipMemcpy on the device failed ({rc})")
    del text
    torch.cuda.synchronize()
    gi = GpuIndex.from_device_codes64(T, isa0, Cf, bw.data_ptr(), T, int(i0.value), Cr, rb.data_ptr())
    assert gi.is64()
    gi.set_sa64_device(sa, sa.n, 32, np.array([[1, 0, T - 1, 0]], U64))
    gi.set_text64_device(d_text, T)
    yield gi, synth.PackedGenome(T, 77)
    gi.close()


def small_side(windows):
    """A fresh small handle whose text is the given code windows laid side by side, 16 zero
    codes between them (the host's MSB-first layout): (index, start of each window)."""
    starts, parts, at = [], [], 0
    for w in windows:
        starts.append(at)
        parts += [np.asarray(w, np.uint8), np.zeros(16, np.uint8)]
        at += len(w) + 16
    codes = np.concatenate(parts)[:at - 16]
    words = np.concatenate([index_io.pack_codes_msb(codes), np.zeros(1, np.uint32)])
    gi = tiny_like("tiny", text=False)
    gi.set_text(words, len(codes))
    return gi, np.array(starts, np.int64)


@pytest.fixture(scope="module")
def big_rows(big_text64):
    """500 reads of 100 bp with one indel of 1-3 bp and up to 2 substitutions from the whole
    text, -n 4 -o 1, max_occ 8, refined."""
    from hsa_amd import synth
    from oracle_ctypes import default_opt
    gi, genome = big_text64
    reads, truth = synth.make_reads(genome, [(0, BIG_T)], 500, 100, 43, indel=True, max_mm_indel=2)
    od = default_opt()
    od.update(max_diff=4, fnr=-1.0, max_gapo=1)
    od["mode"] &= ~0x01
    t, host = search_rows(gi, np.full(500, 100, np.uint32), reads.reshape(-1), od, 8)
    return t, host, refine(gi, t), truth


def test_rows_past_2_32_are_valid(big_text64, big_rows):
    from hsa_amd import _lib
    gi, genome = big_text64
    t, host, out, truth = big_rows
    n = int(host["pos_off"][-1])
    st = out["rows"][:n, 0]
    assert n >= 250 and int(out["ctr"][0]) == n and int(out["ctr"][6]) >= 200
    assert not (st == _lib.HSA_RF_CAP).any() and (st == _lib.HSA_RF_OK).sum() >= 250
    read_of = np.repeat(np.arange(500), np.diff(host["pos_off"]))
    past = found = 0
    for row in np.flatnonzero(st == _lib.HSA_RF_OK):
        j = int(read_of[row])
        rec = host["hits"][int(host["hit_off"][j]) + int(host["pos_hit"][row])]
        replay(out, row, oriented(host, j, int(rec[1] >> 30)), lambda p: genome[p])
        past += int(out["rpos"][row, 0]) >= (1 << 32)
        assert int(out["rpos"][row, 1]) == int(out["rpos"][row, 0]) + 1            # the one block row
        found += int(out["rpos"][row, 0]) == int(truth["start"][j]) and int(out["rows"][row, 1]) == 3
    assert past > 0, "no row past 2^32"
    assert found >= 100, "the refined position of a gapped read is its true start"


def test_rows_past_2_32_equal_their_translation(big_text64, big_rows):
    """The refinement is a function of the read, the strand, the gap count and the text
    window only: every row's window, copied into a small text and refined there at the
    translated position, gives identical outputs, the position shift included.  The SAM
    tests pin the small side to the reference, so this pins the large side."""
    gi, genome = big_text64
    t, host, out, _ = big_rows
    n = int(host["pos_off"][-1])
    pos = host["pos"][:n, 3].astype(np.int64)
    assert (host["pos"][:n, 3] != ONES).all()
    lo = np.maximum(pos - 8, 0)
    hi = np.minimum(pos + 100 + 8 + 8, BIG_T)
    sgi, starts = small_side([genome[np.arange(a, b)] for a, b in zip(lo, hi)])
    small = pos - lo + starts
    p2 = host["pos"].copy()
    p2[:n, 3] = small.astype(U64)
    p2[:n, 2] = (small + 1).astype(U64)
    p2[:n, 0] = p2[:n, 3]
    t2 = dict(t, pos=dev(p2))
    import torch
    torch.cuda.synchronize()
    got = refine(sgi, t2)
    for k in ("rows", "cigar", "md"):
        assert np.array_equal(got[k][:n], out[k][:n]), k
    assert np.array_equal(got["rpos"][:n, 0].astype(np.int64) - small, out["rpos"][:n, 0].astype(np.int64) - pos)
    assert np.array_equal(got["ctr"][:7], out["ctr"][:7])
    sgi.close()


def test_text_end_is_the_same_on_both_sides(big_text64):
    """Rows at the last characters of the text, on the 4.3 Gbp text and on a 400-character
    text that ends the same way: gapped rows whose window the text's end cuts
    (bwtse.c:393), down to one character, and ungapped rows that end at and past it
    (HSA_RF_TEXT).  The two sides must agree; the small side's cut windows are pinned to the
    reference's bwa_refine_gapped by the fixture's `cut` rows (test_golden_rows_equal_the_reference),
    which this test carries past 2^32."""
    from hsa_amd import _lib, synth
    gi, genome = big_text64
    T = BIG_T
    tail = genome[np.arange(T - 400, T)]
    sgi, _ = small_side([tail])
    fw = tail[300:400].copy()
    fw[40] ^= 1
    dl = np.concatenate([tail[298:350], tail[352:400]])                          # a 2 bp deletion, ends at the end
    rv = synth.revcomp_codes(np.concatenate([tail[303:350], [2], tail[350:400], [1, 3]]).astype(np.uint8))
    lens = [100, 100, 100]
    codes = np.concatenate([fw, dl, rv]).astype(np.uint8)
    rows = [(0, 0, 0, 300, 301), (0, 0, 0, 301, 302), (0, 0, 1, 300, 301), (0, 0, 3, 299, 300)]
    rows += [(1, 0, 2, p, p + 1) for p in (298, 299, 300, 330, 399, 400)]
    rows += [(2, 1, g, p, p + 1) for g, p in ((1, 303), (3, 301), (3, 310), (2, 360))]
    sides = []
    for ix, shift in ((sgi, 0), (gi, T - 400)):
        t, _ = fabricate(lens, codes, [(r, s, g, p + shift, o + shift) for r, s, g, p, o in rows])
        sides.append((refine(ix, t), shift))
    (a, _), (b, shift) = sides
    for k in ("rows", "cigar", "md"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["rpos"] + U64(shift), b["rpos"]) and np.array_equal(a["ctr"][:7], b["ctr"][:7])
    st = [int(s) for s in a["rows"][:, 0]]
    assert st[:4] == [0, _lib.HSA_RF_TEXT, 0, 0] and st[4:9] == [0] * 5 and st[9] == _lib.HSA_RF_TEXT and st[10:] == [0] * 4
    assert re.fullmatch(r"\d+M2D\d+M", row_strings(a, 4)["cigar"]) and row_strings(a, 4)["nm"] == 2
    sgi.close()


# ---------------------------------------------------------------- against bwa_refine_gapped itself
@pytest.fixture(scope="module")
def golden_side():
    """A handle whose text is the fixture's text: (index, text)."""
    text = rc.golden()[0]["text"]
    gi, starts = small_side([text])
    assert int(starts[0]) == 0
    yield gi, text
    gi.close()


def golden_batch(rows, per_read=None):
    """fabricate() of fixture rows, one read per row; per_read(r) gives a read's rows as
    (strand, gap, pos, ori) when it has more than its own."""
    lens = [r["len"] for r in rows]
    codes = np.concatenate([r["codes"] for r in rows]).astype(np.uint8)
    per_read = per_read or (lambda r: [(r["strand"], r["gap"], r["pos"], r["ori"])])
    return fabricate(lens, codes, [(k, *x) for k, r in enumerate(rows) for x in per_read(r)])


def differences(out, rows, at=None):
    """The rows of `out` (row at[k] for fixture row k) that are not the reference's, each as
    a line naming the family and both CIGARs."""
    from hsa_amd import _lib, refine as rf
    bad = []
    for k, r in enumerate(rows):
        t = k if at is None else at[k]
        st, n_cigar, nm, md_len, trim5, trim3 = (int(x) for x in out["rows"][t, :6])
        n_ops = min(n_cigar, out["cigar"].shape[1])
        got = dict(status=st, n_cigar=n_cigar, words=[int(w) for w in out["cigar"][t, :n_ops]], nm=nm, md_len=md_len,
                   md=out["md"][t, :min(md_len, out["md"].shape[1])].tobytes(), trim5=trim5, trim3=trim3,
                   rpos=(int(out["rpos"][t, 0]), int(out["rpos"][t, 1])))
        want = dict(status=_lib.HSA_RF_OK, n_cigar=len(r["words"]), words=[int(w) for w in r["words"]], nm=r["nm"],
                    md_len=len(r["md"]), md=r["md"].encode(), trim5=r["trim5"], trim3=r["trim3"],
                    rpos=(r["occ_pos"], r["ori_pos"]))
        if got != want:
            fields = [f for f in want if got[f] != want[f]]
            bad.append(f"case {r['k']} {r['family']} len {r['len']} gap {r['gap']} strand {r['strand']} pos {r['pos']}: "
                       f"device {rf.cigar_text(got['words'])} reference {r['cigar']} (made {r['made'] or '-'}); differ in "
                       + ", ".join(f"{f} {got[f]!r} != {want[f]!r}" for f in fields if f != "words"))
    return bad


def check_against_reference(gi, rows):
    """Every row refined on `gi` is the reference's: status, n_cigar, CIGAR words, NM, md_len,
    MD bytes, trim5 == start, trim3 == len - 1 - end, rpos == (occ_pos, ori_pos).  The strides
    are the set's longest CIGAR and MD, so HSA_RF_MD would be a difference too."""
    t, _ = golden_batch(rows)
    out = refine(gi, t, cigar_stride=max(len(r["words"]) for r in rows), md_stride=max(len(r["md"]) for r in rows))
    assert int(out["ctr"][0]) == len(rows) and int(out["ctr"][6]) == sum(r["gap"] > 0 for r in rows)
    bad = differences(out, rows)
    fams = sorted({b.split()[2] for b in bad})
    assert not bad, f"{len(bad)} of {len(rows)} rows differ from the reference, families {fams}:\n" + "\n".join(bad[:12])
    assert [int(x) for x in out["ctr"][1:6]] == [len(rows), 0, 0, 0, 0]
    return out


def test_golden_rows_equal_the_reference(golden_side):
    """Every row of the committed fixture, none skipped."""
    gi, _ = golden_side
    rows = rc.golden()[2]
    assert len(rows) == 2104
    check_against_reference(gi, rows)


def test_golden_rows_do_not_depend_on_the_layout(golden_side):
    """The 100-base rows in a batch of their own (max_len 100) and in a batch that also holds
    the 1023-base rows (another tb_stride, ring and win_cap): identical outputs, and the
    reference's in both."""
    gi, _ = golden_side
    rows = rc.golden()[2]
    short = [r for r in rows if r["len"] == 100]
    long = [r for r in rows if r["len"] == 1023]
    assert len(short) == 1888 and len(long) == 16
    cs, ms = max(len(r["words"]) for r in rows), max(len(r["md"]) for r in rows)
    ta, _ = golden_batch(short)
    tb, _ = golden_batch(short + long)
    assert ta["max_len"] == 100 and tb["max_len"] == 1023
    a, b = refine(gi, ta, cigar_stride=cs, md_stride=ms), refine(gi, tb, cigar_stride=cs, md_stride=ms)
    n = len(short)
    for k in ("rows", "rpos", "cigar", "md"):
        assert np.array_equal(a[k][:n], b[k][:n]), k
    for out in (a, b):
        bad = differences(out, short)
        assert not bad, f"{len(bad)} rows differ from the reference:\n" + "\n".join(bad[:12])


def test_golden_rows_do_not_depend_on_their_place(golden_side):
    """max_occ-style multiplicity: every 100-base read with three rows -- its own, the same
    position on the other strand, its own again -- so that both strands of one read are
    adjacent in the row list.  Each row answers as it does alone (the same rows, one read
    each), and the read's own rows as the reference does."""
    gi, _ = golden_side
    short = [r for r in rc.golden()[2] if r["len"] == 100]

    def three(r):
        own = (r["strand"], r["gap"], r["pos"], r["ori"])
        return [own, (1 - r["strand"], r["gap"], r["pos"], r["ori"]), own]

    tm, _ = golden_batch(short, per_read=three)
    alone = [dict(r, strand=s, gap=g, pos=p, ori=o) for r in short for s, g, p, o in three(r)]
    t1, _ = golden_batch(alone)
    assert tm["n_jobs"] == len(short) and t1["n_jobs"] == 3 * len(short) == tm["pos_cap"] == t1["pos_cap"]
    # (the other strand's rows are no alignments of anything: their CIGARs run long)
    m, one = refine(gi, tm, cigar_stride=64, md_stride=256), refine(gi, t1, cigar_stride=64, md_stride=256)
    assert same(m, one)
    for slot in (0, 2):
        bad = differences(m, short, at=[3 * k + slot for k in range(len(short))])
        assert not bad, f"{len(bad)} rows differ from the reference:\n" + "\n".join(bad[:12])


@pytest.mark.skipif(not os.path.exists(REF_REFINE), reason="oracle/_ref/ref_refine not built (make -C oracle)")
def test_random_rows_equal_the_reference_run_here(tmp_path):
    """A seeded random set from the same families -- another seed, a text with other motifs
    and stretch lengths, offsets moved, other read lengths -- answered by the reference's
    driver here and compared in the same fields."""
    c = rc.generate(seed=977, vary=True)
    g = rc.golden()[0]
    assert len(c["text"]) != len(g["text"]) and not np.array_equal(c["text"][:1300], g["text"][:1300])
    rows = rc.rows_of(c, rc.run_reference(REF_REFINE, c, str(tmp_path)))
    assert 2000 <= len(rows) <= 2600
    gi, _ = small_side([c["text"]])
    try:
        check_against_reference(gi, rows)
    finally:
        gi.close()
