"""Trimmed reads and barcodes in the SAM lines written on the device
(hsa_sam_lines_device64_trim through hsa_amd.sam.device_sam with full_len / bc) against the
per-read restatement hsa_amd.sam.sam_line with clip_len / bc, on fabricated arrays: both
strands, a CIGAR with and without an S op at the edge bwa_correct_trimmed looks at, the
one-op CIGAR of a read without one, reads with XA rows (whose CIGARs stay); and without the new
inputs the text of before."""
import numpy as np
import pytest

from test_gpu_refine import dev
from test_gpu_sam import CHRS, CS, MAX_TOP2, MS, fabricate, strings, upload

pytestmark = pytest.mark.gpu
BC = 6


@pytest.fixture(scope="module")
def tiny():
    from test_gpu_refine import index_text
    return index_text("tiny")


@pytest.fixture(scope="module")
def batch():
    h = strings(fabricate(600, 31, nohit={5, 77}))
    rng = np.random.default_rng(8)
    full = h["lens"].astype(np.uint32)
    clip = np.array([f if j % 3 == 0 else int(rng.integers(1, f + 1)) for j, f in enumerate(full)], np.uint32)
    bc = rng.choice(np.frombuffer(b"ACGTacgtNn", np.uint8), (h["n"], BC))
    return h, upload(h), full, clip, bc


def line(h, j, clip_len=None, bc=None):
    from hsa_amd import sam
    r0, r1 = int(h["pos_off"][j]), int(h["pos_off"][j + 1])
    o = int(h["jobs"]["off"][j])
    recs = h["hits"][int(h["hit_off"][j]) + h["pos_hit"][r0:r1].astype(np.int64)]
    return sam.sam_line(h["names"][j], h["codes"][o:o + int(h["lens"][j])], h["quals"][j], CHRS, h["sel"][j], h["sel64"][j],
                        h["rows"][r0:r1], h["rpos"][r0:r1], h["cigar"][r0:r1], h["md"][r0:r1], h["pos"][r0:r1], recs,
                        max_top2=MAX_TOP2, clip_len=clip_len, bc=bc) + "\n"


def test_the_batch_covers_the_cases(batch):
    h, _, full, clip, _ = batch
    seen = set()
    for j in range(h["n"]):
        if h["sel"][j, 0] == 0 or clip[j] == full[j]:
            continue
        r0 = int(h["pos_off"][j])
        strand = int(h["hits"][int(h["hit_off"][j]) + int(h["pos_hit"][r0]), 1] >> 30)
        nc = int(h["rows"][r0, 1])
        edge = int(h["cigar"][r0, 0 if strand else nc - 1] >> 28) == 4
        seen.add((strand, edge, nc == 1, int(h["sel"][j, 3]) > 0))
    assert {(s, e) for s, e, _, _ in seen} == {(0, False), (0, True), (1, False), (1, True)}
    assert {(s, one) for s, _, one, _ in seen} >= {(0, True), (1, True)} and any(xa for _, _, _, xa in seen)
    assert (clip == full).sum() >= 200 and (clip == 1).any()


def test_trimmed_reads_and_barcodes(tiny, batch):
    from hsa_amd import sam
    h, d, full, clip, bc = batch
    n = h["n"]
    jobs = h["jobs"].copy()
    jobs["len"] = clip
    m = dict(d, jobs=dev(jobs.view(np.uint8)), n_jobs=n, pos_cap=h["pos_cap"], cigar_stride=CS, md_stride=MS)
    hit = h["sel"][:n, 0] != 0
    for with_bc in (True, False):
        want = "".join(line(h, j, int(clip[j]), bc[j].tobytes() if with_bc else None) for j in range(n) if hit[j]).encode()
        text, off, stat, ctr = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2, full_len=dev(full),
                                              bc=(dev(bc.reshape(-1)), BC) if with_bc else None)
        assert stat.tolist() == [0 if t else 1 for t in hit] and int(ctr[0]) == int(ctr[1]) == len(want)
        if text != want:
            k = next(i for i in range(min(len(text), len(want))) if text[i] != want[i])
            j = int(np.searchsorted(off, k, side="right")) - 1
            raise AssertionError(f"read {j}:\n{text[int(off[j]):int(off[j + 1])]!r}\n{line(h, j, int(clip[j]), bc[j].tobytes())!r}")
        assert text.count(b"\tXC:i:") == int(((clip < full) & hit).sum()) and text.count(b"\tBC:Z:") == (int(hit.sum()) if with_bc else 0)
    again = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2, full_len=dev(full))[0]
    assert again == text                                              # two runs give equal bytes


def test_without_the_new_inputs_the_text_is_todays(tiny, batch):
    from hsa_amd import sam
    h, d, full, _, _ = batch
    n = h["n"]
    m = dict(d, n_jobs=n, pos_cap=h["pos_cap"], cigar_stride=CS, md_stride=MS)
    want = "".join(line(h, j) for j in range(n) if h["sel"][j, 0] != 0).encode()
    plain = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2)
    whole = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2, full_len=dev(full))
    assert plain[0] == want and whole[0] == want and np.array_equal(plain[1], whole[1])
    assert b"\tXC:i:" not in want and b"\tBC:Z:" not in want


def test_bad_trim_arguments(tiny, batch):
    from hsa_amd import sam
    from hsa_amd._lib import HsaError
    h, d, full, clip, bc = batch
    n = h["n"]
    jobs = h["jobs"].copy()
    jobs["len"] = full
    jobs["len"][9] += 1                                                 # searched longer than stored: refused, HSA_SAM_INPUT
    m = dict(d, jobs=dev(jobs.view(np.uint8)), n_jobs=n, pos_cap=h["pos_cap"], cigar_stride=CS, md_stride=MS)
    stat = sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, max_top2=MAX_TOP2, full_len=dev(full))[2]
    assert stat[9] == 4 and (stat[:9] <= 1).all()
    with pytest.raises(HsaError, match="-2"):
        sam.device_sam(tiny, m, h["names"], h["quals"], CHRS, full_len=dev(full), bc=(dev(np.zeros(n * 64, np.uint8)), 64))
