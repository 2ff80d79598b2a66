"""hsa_amd.align with the reader's options (-q, -B, -Y, -I), FASTQ to SAM on the device: every
case of tools/make_golden_opts.py against the compiled reference's committed SAM, whole lines in
the reference's order, the splice path included; batches of 100 and 80 reads (a filtered record
counts towards none); the hand-over between the device loader and the host parser with the
options set; --unaligned with barcodes."""
import io

import pytest

from golden_io import INDEX
from reads_opts_cases import CASES, MANIFEST, case_options, case_reads, case_sam

pytestmark = pytest.mark.gpu
_RUNS = {}


@pytest.fixture(scope="module")
def opened():
    from hsa_amd import align
    gi, chrs = align.open_index64(INDEX["tiny"])
    yield gi, chrs
    gi.close()


def run(opened, args, data, **kw):
    from hsa_amd import align
    gi, chrs = opened
    opts, rest, _ = align.parse_options(args, reader_options=True)
    assert not rest
    out = io.BytesIO()
    state, stats = align.align_fastq(gi, chrs, data, opts, out, **kw)
    return out.getvalue(), state, stats


def case_run(opened, name):
    if name not in _RUNS:
        _RUNS[name] = run(opened, MANIFEST[name]["args"], case_reads(name), splice=True)
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_reference_text(opened, name):
    """Every printed line is a reference line, one per read, in the reference's order; a
    reference line may be missing only for a read the statistics name as refused (handed back,
    more than one pair, a refused spliced line), at most 2 % of the case's lines."""
    from hsa_amd import reads
    mode, trim = case_options(name)
    p = reads.parse_host(case_reads(name), mode=mode, trim_qual=trim)
    want = case_sam(name).split(b"\n")[:-1]
    assert len(want) == MANIFEST[name]["sam_lines"]
    text, _, stats = case_run(opened, name)
    assert text.endswith(b"\n")
    lines = text.split(b"\n")[:-1]
    at = {nm: k for k, nm in enumerate(p["names"])}
    order = [ln.split(b"\t")[0] for ln in lines]
    assert len(set(order)) == len(order) and all(at[a] < at[b] for a, b in zip(order, order[1:]))
    assert stats["reads"] == len(p["names"]) and stats["filtered"] == p["filtered"] and stats["lines"] == len(lines)
    assert stats["trimmed_bases"] == p["trimmed_bases"] and stats["total_bases"] == p["total_bases"]
    assert stats["host_records"] == 0 and stats["device_records"] == len(p["names"])
    where = {ln: k for k, ln in enumerate(want)}
    extra = [ln for ln in lines if ln not in where]
    assert not extra, f"{len(extra)} printed lines are not the reference's, first:\n{extra[0]!r}"
    assert [where[ln] for ln in lines] == sorted(where[ln] for ln in lines)
    have = set(lines)
    missing = [ln for ln in want if ln not in have]
    named = set(stats["refused_names"])
    print(name, dict(lines=len(lines), reference=len(want), missing=len(missing), handed_back=stats["handed_back"],
                     spliced_multi=stats["spliced_multi"], spliced_refused=stats["spliced_refused"], refused=stats["refused"]))
    assert all(ln.split(b"\t")[0] in named for ln in missing)
    assert len(missing) <= stats["handed_back"] + stats["spliced_multi"] + stats["spliced_refused"]
    assert 50 * len(missing) <= len(want)
    assert text.count(b"\tXC:i:") >= MANIFEST[name]["with_XC"] - len(missing)
    assert text.count(b"\tBC:Z:") >= MANIFEST[name]["with_BC"] - len(missing)


def test_the_shifted_file_gives_the_same_text(opened):
    assert case_run(opened, "Iq15")[0] == case_run(opened, "q15")[0]


@pytest.mark.parametrize("batch_reads", [100, 80])
def test_filtered_records_count_towards_no_batch(opened, batch_reads):
    """-n 4 -o 0 fixes the thresholds and opens no gap, so batches differ from one batch only
    in how the reads are cut into them and how the drand48 state travels."""
    args = ["-n", "4", "-o", "0", "-q", "15", "-Y", "-B", "6"]
    data = case_reads("B6q15Y")
    want, want_state, one = run(opened, args, data)
    text, state, stats = run(opened, args, data, batch_reads=batch_reads)
    assert one["batches"] == 1 and one["filtered"] > 40 and want.count(b"\tXC:i:") > 50
    assert stats["batches"] == (one["reads"] + batch_reads - 1) // batch_reads and stats["reads"] == one["reads"]
    assert text == want and state == want_state and stats["filtered"] == one["filtered"]


def test_records_through_the_host_parser(opened):
    """Records 3 and 5 of every 7 with the sequence over two lines: the device loader stops
    there, parse_host takes the record with the same options (those at 3 are the ones the
    Casava filter takes), the loader goes on behind it."""
    ls = case_reads("B6q15Y").split(b"\n")
    recs = []
    for k in range(0, len(ls) - 3, 4):
        h, s, p, q = ls[k:k + 4]
        recs.append(h + b"\n" + (s[:20] + b"\n" + s[20:] if (k // 4) % 7 in (3, 5) else s) + b"\n" + p + b"\n" + q + b"\n")
    text, state, stats = run(opened, MANIFEST["B6q15Y"]["args"], b"".join(recs), splice=True)
    want, want_state, one = case_run(opened, "B6q15Y")
    n = MANIFEST["n"][MANIFEST["B6q15Y"]["reads"]]
    assert text == want and state == want_state and stats["filtered"] == one["filtered"] == len(range(3, n, 7))
    # (asked for one read at a filtered record, parse_host skips it and takes the record behind it, and more
    # at a time where the device loader takes nothing: how many is the driver's business)
    assert stats["host_records"] >= len(range(5, n, 7)) and stats["device_records"] >= 100
    assert stats["device_records"] == one["reads"] - stats["host_records"]


def test_unaligned_reads_keep_their_barcodes(opened):
    from hsa_amd import reads
    un = io.BytesIO()
    data = case_reads("B6q15Y")
    text, _, stats = run(opened, MANIFEST["B6q15Y"]["args"], data, splice=True, unaligned=un)
    assert text == case_run(opened, "B6q15Y")[0]
    mode, trim = case_options("B6q15Y")
    every, kept = reads.parse_host(data), reads.parse_host(data, mode=mode, trim_qual=trim)
    with_line = {ln.split(b"\t")[0] for ln in text.split(b"\n")[:-1]}
    p = reads.parse_host(un.getvalue())
    assert p["names"] == [n for n in kept["names"] if n not in with_line] and len(p["names"]) == stats["no_line"] > 0
    orig = dict(zip(every["names"], zip(every["raw"], every["quals"])))
    assert all((s, q) == orig[n] for n, s, q in zip(p["names"], p["raw"], p["quals"]))      # the record as given: 106 bases
