"""FASTQ to SAM through hsa_amd.align (open_index64, align_fastq): the committed drop-in
reads against the compiled reference's SAM, whole lines in file order; the hand-over between
the device loader and the host parser; the generator's state chained over batches; the index
opened from its files; and a text past 2^32 against device_sam fed from NumPy arrays."""
import gzip
import io
import os

import numpy as np
import pytest

from golden_io import GOLD, INDEX
from test_gpu_choose import chrom_names, reference_lines
from test_gpu_refine import BIG_T, MAN, big_text64, dev, refine, search_rows, tiny_like  # noqa: F401

pytestmark = pytest.mark.gpu
_TEXT = {}


@pytest.fixture(scope="module")
def opened():
    from hsa_amd import align
    gi, chrs = align.open_index64(INDEX["tiny"])
    yield gi, chrs
    gi.close()


def fastq_bytes():
    return gzip.open(os.path.join(GOLD, MAN["reads"])).read()


def run(opened, args, data=None, **kw):
    from hsa_amd import align
    gi, chrs = opened
    opts, rest, _ = align.parse_options(args)
    assert not rest
    out = io.BytesIO()
    state, stats = align.align_fastq(gi, chrs, fastq_bytes() if data is None else data, opts, out, **kw)
    return out.getvalue(), state, stats


def golden_text(opened, name):
    if name not in _TEXT:
        _TEXT[name] = run(opened, MAN[name]["args"])
    return _TEXT[name]


@pytest.mark.parametrize("name,count", [("default", 890), ("n4o0", 526)])
def test_golden_sam_whole_file_order(opened, name, count):
    from hsa_amd import reads
    want = reference_lines(gzip.open(os.path.join(GOLD, f"dropin_ref_{name}.sam.gz")).read())
    assert len(want) == count
    text, _, stats = golden_text(opened, name)
    assert text.endswith(b"\n")
    lines = text.decode().split("\n")[:-1]
    names = [n.decode() for n in reads.parse_host(fastq_bytes())["names"]]
    at = {nm: k for k, nm in enumerate(names)}
    order = [ln.split("\t")[0] for ln in lines]
    assert len(set(order)) == len(order) and all(at[a] < at[b] for a, b in zip(order, order[1:]))   # one line per read, in read order
    assert stats["reads"] == len(names) == MAN["n"] and stats["lines"] == len(lines) and stats["refused"] == 0
    assert stats["host_records"] == 0 and stats["device_records"] == len(names)
    have = set(lines)
    bad = [ln for ln in want if ln not in have]
    assert not bad, f"{len(bad)} of {len(want)} reference lines are not in the text, first:\n{bad[0]}"
    pos = {ln: k for k, ln in enumerate(lines)}
    where = [pos[ln] for ln in want]
    assert where == sorted(where)                                       # in the reference's own order


@pytest.mark.parametrize("name", ["default", "n4o0"])
def test_every_seventh_record_through_the_host_parser(opened, name):
    """The same reads with every 7th record's sequence over two lines: the device loader
    stops there, parse_host takes the record, the loader goes on behind it."""
    ls = fastq_bytes().split(b"\n")
    recs = []
    for k in range(0, len(ls) - 3, 4):
        h, s, p, q = ls[k:k + 4]
        recs.append(h + b"\n" + (s[:20] + b"\n" + s[20:] if (k // 4) % 7 == 3 else s) + b"\n" + p + b"\n" + q + b"\n")
    text, state, stats = run(opened, MAN[name]["args"], data=b"".join(recs))
    want, want_state, _ = golden_text(opened, name)
    assert text == want and state == want_state
    assert stats["host_records"] == len(range(3, MAN["n"], 7)) and stats["device_records"] == MAN["n"] - stats["host_records"]


def test_batches_chain_the_generator_state(opened):
    """-n 4 -o 0: no gap opens, so the GAPE bit the option switch toggles cannot matter, and
    -n 4 fixes the thresholds: batches of 300 reads differ from one batch only in how the
    drand48 state travels."""
    want, want_state, one = golden_text(opened, "n4o0")
    text, state, stats = run(opened, MAN["n4o0"]["args"], batch_reads=300)
    assert one["batches"] == 1 and stats["batches"] == (MAN["n"] + 299) // 300
    assert text == want and state == want_state and state != 0


def test_unaligned_reads_are_written_back(opened):
    from hsa_amd import reads
    un = io.BytesIO()
    text, _, stats = run(opened, MAN["n4o0"]["args"], unaligned=un)
    assert text == golden_text(opened, "n4o0")[0]
    p = reads.parse_host(un.getvalue())
    with_line = {ln.split(b"\t")[0] for ln in text.split(b"\n")[:-1]}
    every = reads.parse_host(fastq_bytes())
    assert len(p["names"]) == stats["no_line"] == MAN["n"] - len(with_line)
    assert p["names"] == [n for n in every["names"] if n not in with_line]


def test_open_index64(opened):
    gi, chrs = opened
    old = tiny_like("tiny")
    assert gi.is64() == old.is64() and chrs == chrom_names("tiny") == ["chr1", "chr2", "chr3"]
    from hsa_amd import index_io
    from oracle_ctypes import default_opt
    text = index_io.read_pac(INDEX["tiny"])
    read = text[70000:70060]
    od = default_opt()
    od.update(max_diff=2, fnr=-1.0)
    od["mode"] &= ~0x01
    a = search_rows(gi, [60], read, od, 4)[1]
    b = search_rows(old, [60], read, od, 4)[1]
    n = int(a["pos_off"][1])
    assert n >= 1 and np.array_equal(a["pos_off"], b["pos_off"]) and np.array_equal(a["pos"][:n], b["pos"][:n])
    assert 70000 in [int(v) for v in a["pos"][:n, 3]]
    ra, rb = refine(gi, search_rows(gi, [60], read, od, 4)[0]), refine(old, search_rows(old, [60], read, od, 4)[0])
    assert np.array_equal(ra["rows"][:n], rb["rows"][:n]) and int(ra["rows"][0, 0]) == 0     # the text is attached
    old.close()


def test_header_lines():
    from hsa_amd import align
    assert align.sam_header(INDEX["tiny"]) == b"@SQ\tSN:chr1\tLN:66667\n@SQ\tSN:chr2\tLN:66667\n@SQ\tSN:chr3\tLN:66669\n"


def test_fastq_past_2_32(big_text64):
    """2 000 synthetic reads written out as FASTQ and aligned through align_fastq: the text
    device_sam gives when it is fed from the NumPy arrays (test_gpu_sam.test_sam_text_past_2_32)."""
    from hsa_amd import align, sam, synth
    from oracle_ctypes import default_opt
    from test_gpu_choose import choose
    gi, genome = big_text64
    n = 2000
    reads_, _ = synth.make_reads(genome, [(0, BIG_T)], n, 100, 47, indel=True, max_mm_indel=2)
    od = default_opt()
    od.update(max_diff=4, fnr=-1.0, max_gapo=1)
    od["mode"] &= ~0x01                                                  # (no GAPE: the option switch changes nothing)
    rng = np.random.default_rng(4)
    given = [f"r{j}/{j % 7}" for j in range(n)]
    quals = [rng.integers(33, 127, 100).astype(np.uint8).tobytes().decode() for _ in range(n)]
    chrs = ["none", "big64"]
    fq = "".join(f"@{given[j]} c\n{''.join('ACGT'[c] for c in reads_[j])}\n+\n{quals[j]}\n" for j in range(n)).encode()
    out = io.BytesIO()
    state, stats = align.align_fastq(gi, chrs, fq, od, out)
    t, host = search_rows(gi, np.full(n, 100, np.uint32), reads_.reshape(-1), od, 1)
    got, sub = choose(gi, t)
    ref = refine(gi, sub)
    m = dict(sub, sel=dev(got["sel"]), sel64=dev(got["sel64"]), rows=dev(ref["rows"]), rpos=dev(ref["rpos"]),
             cigar=dev(ref["cigar"]), md=dev(ref["md"]), cigar_stride=ref["cigar"].shape[1], md_stride=ref["md"].shape[1])
    names = [g[:-2] if g[-2:] in ("/1", "/2") else g for g in given]
    want, _, stat, ctr = sam.device_sam(gi, m, names, quals, chrs, max_top2=od["max_top2"])
    assert out.getvalue() == want and state == got["rng"]
    lines = want.decode().split("\n")[:-1]
    assert len(lines) >= 1500 and stats["lines"] == len(lines) and stats["reads"] == n
    assert any(int(ln.split("\t")[3]) >= (1 << 32) for ln in lines), "no printed position past 2^32"
