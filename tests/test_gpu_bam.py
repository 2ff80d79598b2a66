"""BAM input (-b, -0, -1, -2) through hsa_amd.align and hsa_bam_reads_device alone, on the tiny
index.  The pin: a BAM made of a FASTQ fixture's reads gives the reference's committed SAM for
that FASTQ, byte for byte (the rule of hsa_amd/bam.py: bwa_read_bam without its line 142).
Every input here is valid BAM, the truncated file up to its cut; corrupt bytes are run on the
host only (tests/test_bam_san.py)."""
import gzip
import hashlib
import io
import json
import os

import numpy as np
import pytest

import bam_cases as bm
import bgzf_cases as bc
from golden_io import GOLD, INDEX
from reads_opts_cases import case_reads, case_sam

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLD, "manifest_dropin.json")))
_RUN = {}


@pytest.fixture(scope="module")
def opened():
    from hsa_amd import align
    gi, chrs = align.open_index64(INDEX["tiny"])
    yield gi, chrs
    gi.close()


def run(opened, args, data, **kw):
    from hsa_amd import align
    gi, chrs = opened
    opts, rest, _ = align.parse_options(args, reader_options=True, bam_options=True)
    assert not rest
    out = io.BytesIO()
    state, stats = align.align_fastq(gi, chrs, data, opts, out, **kw)
    return out.getvalue(), state, stats


def dropin_fastq(key):
    return gzip.open(os.path.join(GOLD, MAN[key])).read()


def q15(opened):
    """The FASTQ run every layout is compared with: the q15 fixture's reads, -q 15."""
    if "q15" not in _RUN:
        _RUN["q15"] = run(opened, ["-q", "15"], case_reads("q15"), splice=True)
    return _RUN["q15"]


def all_on_device(stats):
    assert stats["host_records"] == 0 and stats["bam_serial_records"] == 0 and stats["bam_truncated"] == 0
    assert stats["bam_segments_verified"] == stats["bam_segments"] >= 2
    assert stats["inflate_device_blocks"] == stats["inflate_blocks"] >= 3 and stats["inflate_host_blocks"] == 0


# ---------------------------------------------------------------- 1. the pin
@pytest.mark.parametrize("name,reads_key", [("splice_default", "splice_reads"), ("splice_n4o1", "splice_reads"), ("default", "reads")])
def test_dropin_fixtures_give_the_reference_sam(opened, name, reads_key):
    fq = dropin_fastq(reads_key)
    want, want_state, one = run(opened, MAN[name]["args"], fq, splice=True)
    text, state, stats = run(opened, ["-b"] + MAN[name]["args"], bm.aligned(bm.from_fastq(fq)), splice=True)
    print(name, {k: v for k, v in stats.items() if k != "refused_names"})
    assert text == want and state == want_state
    assert hashlib.sha256(text).hexdigest() == MAN[name]["sam_sha256"]
    assert text == gzip.open(os.path.join(GOLD, f"dropin_ref_{name}.sam.gz")).read()
    assert stats["reads"] == one["reads"] and stats["lines"] == MAN[name]["sam_lines"] and stats["device_records"] == one["reads"]
    all_on_device(stats)
    assert set(stats) - set(one) == {"inflate_" + k for k in ("blocks", "device_blocks", "host_blocks", "bytes_in", "bytes_out", "groups")} | \
        {"bam_segments", "bam_segments_verified", "bam_serial_records", "bam_truncated"}


def test_q15_fixture_gives_the_reference_sam(opened):
    want, want_state, one = q15(opened)
    text, state, stats = run(opened, ["-b", "-q", "15"], bm.aligned(bm.from_fastq(case_reads("q15"))), splice=True)
    assert text == want == case_sam("q15") and state == want_state
    assert stats["trimmed_bases"] == one["trimmed_bases"] > 0 and stats["total_bases"] == one["total_bases"]
    all_on_device(stats)


def test_the_fixture_without_options(opened):
    """The q15 fixture's reads without -q, and with the reader options bwa_read_bam ignores."""
    fq = case_reads("q15")
    want, want_state, _ = run(opened, [], fq, splice=True)
    data = bm.aligned(bm.from_fastq(fq))
    text, state, stats = run(opened, ["-b"], data, splice=True)
    assert text == want and state == want_state and b"\tXC:i:" not in text
    all_on_device(stats)
    ignored = run(opened, ["-b", "-B", "6", "-I", "-Y"], data, splice=True)
    assert ignored[:2] == (want, want_state) and b"\tBC:Z:" not in ignored[0]
    # -0 without -b: the file is opened as FASTQ
    assert run(opened, ["-0", "-1"], fq, splice=True)[:2] == (want, want_state)


# ---------------------------------------------------------------- 2. layouts
LAYOUTS = {"aligned65280": lambda r: bm.aligned(r, 65280), "aligned4096": lambda r: bm.aligned(r, 4096),
           "aligned600": lambda r: bm.aligned(r, 600), "straddling4096": lambda r: bm.straddling(r, 4096),
           "straddling512": lambda r: bm.straddling(r, 512), "one_stream": bm.one_stream, "uncompressed": bm.text_of}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts_give_the_same_text(opened, layout, tmp_path):
    want, want_state, one = q15(opened)
    data = LAYOUTS[layout](bm.from_fastq(case_reads("q15")))
    if layout == "aligned4096":                              # (once from a path)
        (tmp_path / "reads.bam").write_bytes(data)
        data = str(tmp_path / "reads.bam")
    text, state, stats = run(opened, ["-b", "-q", "15"], data, splice=True)
    print(layout, {k: v for k, v in stats.items() if k.startswith(("bam_", "inflate_", "host", "device"))})
    assert text == want and state == want_state and stats["reads"] == one["reads"] and stats["host_records"] == 0
    if layout.startswith("aligned"):
        assert stats["bam_serial_records"] == 0 and stats["bam_segments_verified"] == stats["bam_segments"]
        if layout == "aligned600":
            assert stats["bam_segments"] > one["reads"] // 3
    else:
        assert stats["bam_serial_records"] > 0
    if layout in ("one_stream", "uncompressed"):
        assert stats["inflate_blocks"] == 0 and stats["bam_serial_records"] == one["reads"]


# ---------------------------------------------------------------- 3. a record larger than its members
def test_a_record_larger_than_its_members(opened):
    """One 3 000-base read among 100-base reads, members of 1 024 bytes: anchors fall inside
    the record.  The long read starts with 15 A, so the reader keeps it and the search's
    poly-A test leaves it out: what is checked is the walk across it."""
    rng = np.random.default_rng(7)
    long_seq = b"A" * 15 + bytes(rng.choice(list(b"ACGT"), 2985).tolist())
    recs = bm.from_fastq(case_reads("q15"))[:120]
    recs.insert(50, bm.record(b"long3000", long_seq, bytes(rng.integers(2, 41, 3000).tolist())))
    args = ["-b", "-n", "4", "-o", "0"]
    want, want_state, one = run(opened, args, bm.aligned(recs, 65280))
    text, state, stats = run(opened, args, bm.aligned(recs, 1024))
    assert text == want and state == want_state and stats["reads"] == one["reads"] == 121 and one["polyat"] >= 1
    assert stats["host_records"] == 0
    assert stats["bam_serial_records"] > 0 and stats["bam_segments_verified"] < stats["bam_segments"]
    assert len(text.split(b"\n")) > 60


# ---------------------------------------------------------------- 4. batches
@pytest.mark.parametrize("batch_reads", [100, 97])
def test_batches(opened, batch_reads):
    """-n 4 -o 0 fixes the thresholds and opens no gap, so batches differ from one batch only in
    how the reads are cut into them; every fourth record is skipped by -0 and counts towards none."""
    fq = case_reads("q15")
    n = len(fq.split(b"\n")) // 4
    flags = [bm.FLAG_READ1 if k % 4 == 1 and k < n - 1 else 0 for k in range(n)]
    data = bm.aligned(bm.from_fastq(fq, flags), 4096)
    args = ["-b", "-0", "-n", "4", "-o", "0", "-q", "15"]
    want, want_state, one = run(opened, args, data)
    text, state, stats = run(opened, args, data, batch_reads=batch_reads)
    kept = n - len(range(1, n - 1, 4))
    assert one["batches"] == 1 and one["reads"] == kept and one["filtered"] == n - kept
    assert stats["batches"] == (kept + batch_reads - 1) // batch_reads and stats["reads"] == kept and stats["filtered"] == n - kept
    assert text == want and state == want_state and len(text) > 10000


# ---------------------------------------------------------------- 5. selection
@pytest.mark.parametrize("opt,bit", [("-1", 1), ("-2", 2), ("-0", 4)])
def test_selection(opened, opt, bit):
    fq = case_reads("q15")
    n = len(fq.split(b"\n")) // 4
    cls = [(1, bm.FLAG_READ1), (2, bm.FLAG_READ2), (4, 0)]
    data = bm.aligned(bm.from_fastq(fq, [cls[k % 3][1] for k in range(n)]), 4096)
    want, want_state, one = run(opened, [], bm.fastq_of(fq, lambda k: cls[k % 3][0] == bit))
    text, state, stats = run(opened, ["-b", opt], data)
    assert text == want and state == want_state and stats["reads"] == one["reads"] == len(range({1: 0, 2: 1, 4: 2}[bit], n, 3))
    assert stats["filtered"] == n - one["reads"] and len(text) > 5000


# ---------------------------------------------------------------- 6. -q 15 with reversed records
def test_trimming_walks_from_the_reads_own_end(opened):
    """Every third record is stored reversed (FLAG 0x10): its low-quality end is the front of
    the stored qualities.  XC:i and the clipped CIGAR as the committed q15 SAM has them."""
    from reads_opts_cases import sam_fields
    from hsa_amd import reads
    fq = case_reads("q15")
    names = reads.parse_host(fq)["names"]
    reversed_names = {nm for k, nm in enumerate(names) if k % 3 == 2}
    text, _, _ = run(opened, ["-b", "-q", "15"], bm.aligned(bm.from_fastq(fq), 4096), splice=True)
    got = {ln.split(b"\t")[0]: sam_fields(ln) for ln in text.split(b"\n")[:-1]}
    want = {ln.split(b"\t")[0]: sam_fields(ln) for ln in case_sam("q15").split(b"\n")[:-1]}
    clipped = [nm for nm in want if nm in reversed_names and b"XC" in want[nm]["tags"]]
    assert len(clipped) >= 20
    for nm in clipped:
        assert got[nm]["tags"][b"XC"] == want[nm]["tags"][b"XC"] and got[nm]["cigar"] == want[nm]["cigar"], nm
        assert got[nm]["seq"] == want[nm]["seq"] and got[nm]["qual"] == want[nm]["qual"], nm


# ---------------------------------------------------------------- 7. the loader alone
def loader_records():
    """The small fixture reads (lengths odd and even), the edge records, and a 3 000-base read."""
    rng = np.random.default_rng(11)
    long_rec = bm.record(b"long3000", bytes(rng.choice(list(b"ACGT"), 3000).tolist()), bytes(rng.integers(0, 60, 3000).tolist()),
                         bm.FLAG_UNMAPPED | bm.FLAG_REVERSE)
    fq = bm.from_fastq(bm.small_fastq())
    return fq[:7] + bm.edge_records() + [long_rec] + fq[7:] + bm.from_fastq(case_reads("q15"))[:150]


def load(gi, text, anchors=(0,), at_eof=True, max_records=1 << 20, which=7, trim_qual=0, table=None, **kw):
    import torch
    from hsa_amd import bam
    d = torch.from_numpy(np.frombuffer(text, np.uint8).copy() if len(text) else np.zeros(1, np.uint8)).cuda()
    return bam.load_device(gi, d, len(text), at_eof, max_records, 4, 32, anchors=anchors, which=which, trim_qual=trim_qual,
                           maxdiff=table, **kw)


def check_against_host(t, text, which=7, trim_qual=0, table=None, max_records=None):
    """Rows, jobs, codes, names, qualities, full_len and counters of a load_device result
    against bam.parse_host through align._host_segment."""
    from hsa_amd import align, bam
    from hsa_amd._lib import HSA_RD_FILTERED, JOB_DTYPE
    p = bam.parse_host(text, max_records, which=which, trim_qual=trim_qual)
    md_of = (lambda l: int(table[l])) if table is not None else (lambda l: 4)
    h = align._host_segment(p, md_of(max(p["lens"], default=0)), md_of, 32)
    n, c = len(h["jobs"]), t["ctr"]
    rec = t["rec"][:4 * t["n_rows"]].cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert t["n_loaded"] == len(p["names"]) and t["n_rows"] == len(p["names"]) + p["filtered"] and c["consumed"] == p["consumed"]
    assert t["octr"] == dict(rows=t["n_rows"], filtered=p["filtered"], trimmed_bases=p["trimmed_bases"], total_bases=p["total_bases"])
    assert (rec[rec[:, 0] == HSA_RD_FILTERED][:, 1:3] == 0).all()
    assert np.array_equal(rec[rec[:, 0] != HSA_RD_FILTERED], h["rec"])
    assert t["n_jobs"] == n == c["jobs_wanted"] and c["code_wanted"] == len(h["codes"]) + 16
    assert np.array_equal(t["jobs"][:n * JOB_DTYPE.itemsize].cpu().numpy().view(JOB_DTYPE), h["jobs"])
    codes = t["codes"][:len(h["codes"]) + 16].cpu().numpy()
    assert np.array_equal(codes[:-16], h["codes"]) and not codes[-16:].any()
    assert t["names"][:c["name_wanted"]].cpu().numpy().tobytes() == h["names"].tobytes()
    assert t["quals"][:c["qual_wanted"]].cpu().numpy().tobytes() == h["quals"].tobytes()
    assert np.array_equal(t["name_off"][:n + 1].cpu().numpy().view(np.uint64), h["name_off"])
    assert np.array_equal(t["qual_off"][:n + 1].cpu().numpy().view(np.uint64), h["qual_off"])
    assert np.array_equal(t["full_len"][:n].cpu().numpy().view(np.uint32), h["full_len"])
    assert c["max_loaded"] == max(p["lens"], default=0) and c["threshold"] == md_of(c["max_loaded"]) & 0xFFFFFFFFFFFFFFFF
    return p


def member_anchors(recs, member):
    """The anchors align passes for the aligned layout: the members' output offsets behind 0."""
    from hsa_amd import bgzf
    t = bgzf.scan(bm.aligned(recs, member, head=b""))
    return [0] + [int(v) for v in np.unique(t["out_off"][t["isize"] > 0]) if v > 0]


@pytest.mark.parametrize("trim_qual,use_table", [(0, False), (15, False), (15, True)])
def test_loader_against_parse_host(opened, trim_qual, use_table):
    import torch
    from hsa_amd import align
    from hsa_amd._lib import HSA_BAM_END_ANCHOR, HSA_BAM_END_INPUT, HSA_BAM_END_MAX
    gi = opened[0]
    recs = loader_records()
    text = b"".join(recs)
    tab = align._table(0.04) if use_table else None
    d_tab = torch.from_numpy(tab).cuda() if use_table else None
    kw = dict(trim_qual=trim_qual, table=d_tab)
    for member in (65280, 8192, 4096, 600):
        anchors = member_anchors(recs, member)
        t = load(gi, text, anchors, **kw)
        if member <= 4096:                                  # the anchors inside the long record (4 5xx bytes) are not on the chain
            assert t["bctr"]["reason"] == HSA_BAM_END_ANCHOR and 0 < t["bctr"]["segments_verified"] < len(anchors) - 1
            at = t["consumed"]
            check_against_host(t, text[:at], trim_qual=trim_qual, table=tab)
            rest = load(gi, text[at:], [0] + [a - at for a in anchors if a > at], **kw)
            check_against_host(rest, text[at:], trim_qual=trim_qual, table=tab)
            assert rest["bctr"]["reason"] == HSA_BAM_END_INPUT and t["n_rows"] + rest["n_rows"] == len(recs)
        else:
            check_against_host(t, text, trim_qual=trim_qual, table=tab)
            assert t["bctr"]["reason"] == HSA_BAM_END_INPUT
            assert t["bctr"]["segments_verified"] == len(anchors) == {65280: 1, 8192: 5}[member]
            assert t["bctr"]["chain_records"] == len(recs)
    one = load(gi, text, **kw)
    p = check_against_host(one, text, trim_qual=trim_qual, table=tab)
    assert one["bctr"] == dict(reason=HSA_BAM_END_INPUT, segments_verified=1, chain_records=len(recs), chain_end=len(text))
    assert len(p["names"]) == len(recs) - 1 and {len(s) % 2 for s in p["seqs"]} == {0, 1} and max(p["lens"]) > 2000
    # anchors that are not record starts: exact up to the first one, then the caller's turn
    ends = np.cumsum([len(r) for r in recs])
    assert 1000 not in ends
    cut = load(gi, text, [0, 1000, 1001, 5000], **kw)
    assert cut["bctr"]["reason"] == HSA_BAM_END_ANCHOR and cut["bctr"]["segments_verified"] == 0
    assert cut["consumed"] == int(ends[ends > 1000][0])
    check_against_host(cut, text[:cut["consumed"]], trim_qual=trim_qual, table=tab)
    # max_records counts reads, not records
    few = load(gi, text, member_anchors(recs, 8192), max_records=11, **kw)
    assert few["bctr"]["reason"] == HSA_BAM_END_MAX and few["n_loaded"] == 11 and few["n_rows"] == 12      # (the empty record)
    check_against_host(few, text, trim_qual=trim_qual, table=tab, max_records=11)
    # two runs give equal arrays
    again, once_more = load(gi, text, member_anchors(recs, 8192), **kw), load(gi, text, member_anchors(recs, 8192), **kw)
    for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "full_len", "rec"):
        assert torch.equal(again[k], once_more[k]), k


@pytest.mark.parametrize("every", [4096, 512])
def test_loader_with_the_anchors_of_a_straddling_cut(opened, every):
    """The anchors a file cut every `every` bytes regardless of records gives: the call is exact
    up to the first anchor that is not a record start and says so; from there on the single
    anchor, as align goes on, gives the rest."""
    from hsa_amd import bgzf
    from hsa_amd._lib import HSA_BAM_END_ANCHOR, HSA_BAM_END_INPUT
    recs = loader_records()
    text = b"".join(recs)
    t = bgzf.scan(bm.straddling(recs, every, head=b""))
    anchors = [int(v) for v in np.unique(t["out_off"][t["isize"] > 0])]
    ends = np.cumsum([len(r) for r in recs])
    assert anchors[0] == 0 and len(anchors) > 8 and anchors[1] not in ends
    first = load(opened[0], text, anchors)
    assert first["bctr"]["reason"] == HSA_BAM_END_ANCHOR and first["bctr"]["segments_verified"] == 0
    at = first["consumed"]
    assert at == int(ends[ends > anchors[1]][0])
    check_against_host(first, text[:at])
    rest = load(opened[0], text[at:])
    check_against_host(rest, text[at:])
    assert rest["bctr"]["reason"] == HSA_BAM_END_INPUT and first["n_rows"] + rest["n_rows"] == len(recs)


@pytest.mark.parametrize("which", [1, 2, 3, 4, 5, 6])
def test_loader_selection(opened, which):
    text = b"".join(bm.edge_records() + bm.from_fastq(bm.small_fastq()))
    check_against_host(load(opened[0], text, which=which), text, which=which)


def test_loader_with_short_capacities(opened):
    """Too-small capacities: wanted > written, nothing past a capacity is touched, the repeat
    (load_device's second run) is equal to a run with room."""
    import torch
    from hsa_amd import bam
    from hsa_amd._lib import BamBatch, JOB_DTYPE, RD_COUNTERS
    gi = opened[0]
    text = b"".join(loader_records())
    full = load(gi, text)
    caps = dict(jobs=10, codes=777, names=33, quals=501)
    t = load(gi, text, caps=caps)                           # (runs again with the counters' sizes)
    for k in ("jobs", "codes", "names", "quals", "name_off", "qual_off", "full_len"):
        n = min(len(t[k]), len(full[k]))
        assert torch.equal(t[k][:n], full[k][:n]), k
    assert t["ctr"] == full["ctr"]
    # the first call alone, with guard bytes behind every capacity
    G = 64
    d_in = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    mk = lambda n: torch.full((n + G,), 0xEE, dtype=torch.uint8, device="cuda")
    o = dict(jobs=mk(caps["jobs"] * JOB_DTYPE.itemsize), codes=mk(caps["codes"]), names=mk(caps["names"]), quals=mk(caps["quals"]),
             name_off=mk((caps["jobs"] + 1) * 8), qual_off=mk((caps["jobs"] + 1) * 8), full_len=mk(caps["jobs"] * 4))
    rows = len(text) // 37 + 1
    rec = torch.zeros(rows * 4, dtype=torch.int32, device="cuda")
    ctr, octr, bctr = (torch.zeros(n, dtype=torch.int64, device="cuda") for n in (16, 4, 4))
    anchor = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gi.bam_reads_device(BamBatch(d_in=d_in.data_ptr(), n_in=len(text), at_eof=1, max_records=1 << 20, which=7, trim_qual=0, max_diff=4,
                                 d_maxdiff=None, n_maxdiff=0, len_floor=0, seed_len=32, regime=0, d_anchor=anchor.data_ptr(),
                                 n_anchor=1, d_jobs=o["jobs"].data_ptr(), job_cap=caps["jobs"], d_codes=o["codes"].data_ptr(),
                                 code_cap=caps["codes"], d_names=o["names"].data_ptr(), name_cap=caps["names"],
                                 d_name_off=o["name_off"].data_ptr(), d_quals=o["quals"].data_ptr(), qual_cap=caps["quals"],
                                 d_qual_off=o["qual_off"].data_ptr(), d_full_len=o["full_len"].data_ptr(), d_rec=rec.data_ptr(),
                                 rec_cap=rows, d_counters=ctr.data_ptr(), d_opt_counters=octr.data_ptr(),
                                 d_bam_counters=bctr.data_ptr()))
    torch.cuda.synchronize()
    c = dict(zip(RD_COUNTERS, (int(v) for v in ctr.cpu().numpy().view(np.uint64))))
    assert c["jobs_wanted"] == full["n_jobs"] > c["jobs_written"] == 10 and c["code_wanted"] > c["code_written"] == 777
    assert c["name_wanted"] > c["name_written"] == 33 and c["qual_wanted"] > c["qual_written"] == 501
    for k, v in o.items():
        assert (v[-G:] == 0xEE).all(), k
    assert torch.equal(o["codes"][:777], full["codes"][:777]) and torch.equal(o["quals"][:501], full["quals"][:501])
    assert torch.equal(o["names"][:33], full["names"][:33])


def test_loader_mid_record_cut_without_eof(opened):
    from hsa_amd._lib import HSA_BAM_END_INCOMPLETE, HSA_BAM_END_INPUT
    recs = bm.from_fastq(bm.small_fastq())
    text = b"".join(recs)
    whole = sum(len(r) for r in recs[:8])
    for extra in (1, 20, 40, len(recs[8]) - 1):
        t = load(opened[0], text[:whole + extra], at_eof=False)
        assert t["consumed"] == whole and t["n_loaded"] == 8 and t["bctr"]["reason"] == HSA_BAM_END_INCOMPLETE, extra
        check_against_host(t, text[:whole])
    t = load(opened[0], text[:whole], at_eof=False)
    assert t["consumed"] == whole and t["bctr"]["reason"] == HSA_BAM_END_INPUT and t["bctr"]["segments_verified"] == 1
    assert load(opened[0], b"")["bctr"]["reason"] == HSA_BAM_END_INPUT


def test_loader_argument_errors(opened):
    import torch
    from hsa_amd import bam
    from hsa_amd._lib import BamBatch, HsaError
    gi = opened[0]
    text = b"".join(bm.from_fastq(bm.small_fastq()))
    for kw in (dict(which=0), dict(which=8)):
        with pytest.raises(HsaError):
            load(gi, text, **kw)
    for anchors in ((), (5,), (0, 300, 200), (0, len(text) + 1)):
        with pytest.raises(ValueError, match="anchors"):
            load(gi, text, anchors)
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    ok = dict(d_in=z.data_ptr(), n_in=0, at_eof=1, max_records=4, which=7, d_anchor=z.data_ptr(), n_anchor=1, d_name_off=z.data_ptr(),
              d_qual_off=z.data_ptr(), d_full_len=z.data_ptr(), d_rec=z.data_ptr(), d_counters=z.data_ptr(), d_opt_counters=z.data_ptr(),
              d_bam_counters=z.data_ptr())
    torch.cuda.synchronize()
    gi.bam_reads_device(BamBatch(**ok))
    torch.cuda.synchronize()
    for bad in (dict(n_anchor=0), dict(d_anchor=None), dict(d_counters=None), dict(d_bam_counters=None), dict(d_rec=None),
                dict(n_in=(1 << 32) - 256), dict(n_in=8, d_in=None), dict(max_records=0), dict(at_eof=2), dict(job_cap=1)):
        with pytest.raises(HsaError):
            gi.bam_reads_device(BamBatch(**dict(ok, **bad)))
    # the FASTQ calls keep refusing the BAM bits
    from hsa_amd import reads
    for bit in (0x20, 0x40, 0x80, 0x100):
        with pytest.raises(HsaError):
            reads.load_device(gi, reads.upload(b"@r\nACGT\n+\nIIII\n"), 15, True, 4, 4, 32, mode=bit)


# ---------------------------------------------------------------- 8. the hand-over
def test_records_through_the_host_parser(opened):
    """Every 7th record with an empty name: the device loader stops there, bam.parse_host takes
    the record, the loader goes on behind it.  The text is that of the run where the same
    records have names, the names taken out."""
    fq = case_reads("q15")
    recs, plain = bm.from_fastq(fq)[:200], bm.from_fastq(fq)[:200]
    for k in range(3, 200, 7):
        body = recs[k][4:]
        l_name = body[8]
        # the name field becomes a lone NUL: shorter by l_name - 1
        new = body[:8] + b"\x01" + body[9:32] + b"\0" + body[32 + l_name:]
        recs[k] = len(new).to_bytes(4, "little") + new
        marked = body[:32] + b"~" * (l_name - 1) + b"\0" + body[32 + l_name:]
        plain[k] = len(marked).to_bytes(4, "little") + marked
    args = ["-b", "-n", "4", "-o", "0", "-q", "15"]
    want, want_state, one = run(opened, args, bm.aligned(plain, 4096))
    text, state, stats = run(opened, args, bm.aligned(recs, 4096))
    lines = [b"" + ln[ln.index(b"\t"):] if ln.startswith(b"~") else ln for ln in want.split(b"\n")]
    assert any(ln.startswith(b"~") for ln in want.split(b"\n")) and text == b"\n".join(lines) and state == want_state
    assert one["host_records"] == 0 and stats["host_records"] >= len(range(3, 200, 7))
    assert stats["device_records"] == 200 - stats["host_records"] and stats["reads"] == 200


def test_a_read_past_the_maxdiff_table_is_handed_over(opened):
    """With -n 0.04 a read of TABLE_LEN bases or more is the host's: the batch loader gives a
    device segment, a host segment with that read, and a device segment behind it."""
    import collections
    import torch
    from hsa_amd import align, bam
    gi = opened[0]
    recs = bm.from_fastq(case_reads("q15"))[:60]
    recs.insert(20, bm.record(b"long4100", b"N" * 4100, bytes([30] * 4100)))
    data = bm.aligned(recs, 4096)
    text, d_text, cand, _ = bam.open_text(gi, data)
    opt = align.parse_options(["-n", "0.04"])[0]
    opt["trim_qual"] = 0
    stats = collections.Counter()
    src = dict(text=text, d_text=d_text, cand=cand, which=7)
    segs, pos, _ = align._load_batch_bam(gi, src, bam.read_header(text)[0], opt, torch.from_numpy(align._table(0.04)).cuda(), 1000,
                                         1 << 20, stats)
    assert pos == len(text) and [s["kind"] for s in segs] == ["dev", "host", "dev"]
    assert segs[0]["t"]["n_loaded"] == 20 and segs[1]["p"]["names"] == [b"long4100"] and segs[2]["t"]["n_loaded"] == 40
    assert len(segs[1]["p"]["seqs"][0]) == 4100 and stats["bam_truncated"] == 0


def test_a_read_past_the_maxdiff_table_end_to_end(opened, monkeypatch):
    """-n 0.04 and one read of 4 100 N among 100-base reads: the read goes through the host
    parser and sets the batch's threshold (bwa_cal_maxdiff(4100) = 25), wider than the one the
    device segments took from their own longest read (5).  Record 5 holds 8 N: dropped by its
    segment's threshold, kept by the batch's, so _merge turns that device segment into a host
    segment (bam.parse_host over the bytes the call consumed).  The text is the FASTQ run's."""
    from hsa_amd import bam
    ls = case_reads("q15").split(b"\n")
    recs = [ls[4 * k:4 * k + 4] for k in range(60)]
    recs[5][1] = recs[5][1][:40] + b"N" * 8 + recs[5][1][48:]
    recs.insert(20, [b"@long4100", b"N" * 4100, b"+", b"I" * 4100])
    fq = b"".join(b"\n".join(r) + b"\n" for r in recs)
    want, want_state, one = run(opened, ["-n", "0.04"], fq)
    calls = []
    real = bam.parse_host
    monkeypatch.setattr(bam, "parse_host", lambda *a, **k: calls.append((a[1] if len(a) > 1 else k.get("max_records"), k.get("start", 0))) or real(*a, **k))
    text, state, stats = run(opened, ["-b", "-n", "0.04"], bm.aligned(bm.from_fastq(fq), 4096))
    assert text == want and state == want_state and len(text) > 3000
    assert {k: stats[k] for k in ("reads", "searched", "n_drop", "lines")} == {k: one[k] for k in ("reads", "searched", "n_drop", "lines")}
    assert stats["reads"] == 61 and stats["n_drop"] >= 1 and stats["host_records"] == 1 and stats["device_records"] == 60
    assert (None, 0) in calls, "no device segment was converted"


# ---------------------------------------------------------------- 9. a truncated file
def test_a_truncated_file(opened, tmp_path, capsys):
    """The last record is cut (valid up to the cut): the lines of the reads before it,
    bam_truncated == 1, and main returns 1."""
    from hsa_amd import align
    recs = bm.from_fastq(case_reads("q15"))[:80]
    args = ["-b", "-n", "4", "-o", "0"]
    want, want_state, one = run(opened, args, bm.aligned(recs[:79], 4096))
    cut = bm.text_of(recs)[:-30]
    data = bc.bgzf_file(cut, block=4096)
    text, state, stats = run(opened, args, data)
    assert text == want and state == want_state and stats["bam_truncated"] == 1 and one["bam_truncated"] == 0
    assert stats["reads"] == 79 and len(want) > 5000
    p = tmp_path / "cut.bam"
    p.write_bytes(data)
    out = tmp_path / "out.sam"
    assert align.main(args + ["-f", str(out), INDEX["tiny"], str(p)]) == 1
    assert out.read_bytes() == want and "truncated" in capsys.readouterr().err
    good = tmp_path / "good.bam"
    good.write_bytes(bm.aligned(recs[:79], 4096))
    assert align.main(args + ["-f", str(out), INDEX["tiny"], str(good)]) == 0 and out.read_bytes() == want


def test_unaligned_reads_are_written_in_their_own_orientation(opened):
    from hsa_amd import reads
    fq = case_reads("q15")
    un = io.BytesIO()
    args = ["-b", "-n", "4", "-o", "0"]
    text, _, stats = run(opened, args, bm.aligned(bm.from_fastq(fq), 4096), unaligned=un)
    with_line = {ln.split(b"\t")[0] for ln in text.split(b"\n")[:-1]}
    every, p = reads.parse_host(fq), reads.parse_host(un.getvalue())
    assert p["names"] == [n for n in every["names"] if n not in with_line] and len(p["names"]) == stats["no_line"] > 0
    orig = dict(zip(every["names"], zip(every["raw"], every["quals"])))
    assert all((s, q) == (orig[n][0].upper(), orig[n][1]) for n, s, q in zip(p["names"], p["raw"], p["quals"]))
