"""The refinement's reference-answered fixture (tests/golden/refine_cases.npz), guarded on the
CPU: the file's inputs are what tests/refine_cases.py generates, the compiled reference
(where oracle/_ref/ref_refine is built) still gives the file's answers, every answered row
replays against the text, and a census of what the file holds."""
import os

import numpy as np
import pytest

import refine_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_refine")


def test_fixture_inputs_are_the_generated_cases():
    c, _, _ = rc.golden()
    g = rc.cases()
    for k in rc.INPUTS:
        assert c[k].dtype == g[k].dtype and np.array_equal(c[k], g[k]), k
    again = rc.generate()                                        # seeded: two runs, one set
    assert all(np.array_equal(again[k], g[k]) for k in rc.INPUTS)
    other = rc.generate(seed=rc.SEED + 1, vary=True)             # the live comparison's set is another one
    assert not np.array_equal(other["text"][:1300], g["text"][:1300])


def test_cases_stay_inside_the_contract():
    from hsa_amd import _lib
    c, _, rows = rc.golden()
    T = len(c["text"])
    assert 2000 <= T <= 5000 and int(c["text"].max()) <= 3
    assert int(c["lens"].min()) == 1 and int(c["lens"].max()) == 1023 <= _lib.HSA_RF_MAX_LEN
    assert int(c["gap"].max()) == 16 <= _lib.HSA_RF_MAX_GAP
    assert (c["pos"] < T).all() and int(c["codes"].max()) == 4 and len(c["codes"]) == int(c["lens"].sum())
    ungapped = c["gap"] == 0
    assert (c["pos"][ungapped].astype(np.int64) + c["lens"][ungapped] <= T).all()     # past the end: HSA_RF_TEXT, not a case
    assert set(int(v) for v in c["pos"][ungapped] % 16) == set(range(16))
    assert set(int(v) for v in c["pos"][~ungapped] % 16) == set(range(16)) and int(c["pos"].min()) == 0
    assert set(rc.ODD_LENS) <= set(int(v) for v in c["lens"])
    keeps = {T - r["pos"] for r in rows if r["family"] == "cut"}
    assert keeps == set(rc.CUT_KEEPS)


@pytest.mark.skipif(not os.path.exists(DRIVER), reason="oracle/_ref/ref_refine not built (make -C oracle)")
def test_reference_still_gives_the_fixture_answers(tmp_path):
    c, a, _ = rc.golden()
    got = rc.run_reference(DRIVER, c, str(tmp_path))
    for k in rc.ANSWERS:
        assert got[k].dtype == a[k].dtype and np.array_equal(got[k], a[k]), k


def test_every_fixture_row_replays():
    """The CIGAR spans the read and ends inside the window, NM and MD spell the text; the
    position moved by the trimmed deletion, on both coordinates; a row without a gap has no
    CIGAR of the reference's."""
    c, a, rows = rc.golden()
    text = c["text"]
    assert len(rows) == len(c["lens"]) == len(a["head"])
    for r in rows:
        span, nm, md, x_end = rc.replay(r, text)
        assert (span, nm, md) == (r["len"], r["nm"], r["md"]), (r["k"], r["family"], r["cigar"], r["md"], md)
        window = min(r["len"] + r["gap"], len(text) - r["pos"])
        if r["gap"]:
            assert x_end + r["trim3"] == r["pos"] + window, (r["k"], r["family"], r["cigar"])
        assert r["trim5"] >= 0 and r["trim3"] >= 0
        assert r["occ_pos"] == r["pos"] + r["trim5"] and r["ori_pos"] == r["ori"] + r["trim5"]
        assert (int(a["head"][r["k"], 5]) == 0) == (r["gap"] == 0)


def test_fixture_census():
    """What the file holds, as exact numbers taken from the generated fixture: a later edit
    cannot hollow it out.  `moved`: rows whose CIGAR is not the events where they were made --
    the ties are live."""
    _, _, rows = rc.golden()
    assert rc.census(rows) == dict(rows=2104, gapped=1982, trim5=273, trim3=694, lead_s=34, trail_s=154, moved=1149,
                                   del14=280, cut=168, forward=1052, reverse=1052)
    fam = {}
    for r in rows:
        f = r["family"].split("_")[0]
        fam[f] = fam.get(f, 0) + 1
    assert fam == dict(ties=512, chunk=240, carried=234, ends5=168, ends3=168, declared=136, two=60, n=72, lengths=180, longest=4,
                       cut=174, addressing=68, ungapped=88)
    # the chunk family's long deletions that the reference moves across the band's first 64 columns
    assert sum(r["family"] == "chunk_di" and r["gap"] >= 14 and r["cigar"] != r["made"] for r in rows) == 40
    assert max(len(r["words"]) for r in rows) == 11 and max(len(r["md"]) for r in rows) == 35
