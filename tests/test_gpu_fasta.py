"""FASTA bytes to the packed texts and the annotation tables on the device
(hsa_fasta_device), and a BWT to its .bwt / .fmv bodies (hsa_bwt_files_device), against the
host functions of hsa_amd/index_build.py and index_io.py byte for byte: the committed index
files, hand-written edge records, the length quirks, tile edges under every placement of the
input, seeded random inputs, refused inputs, short capacities and guard bytes, bad
arguments; build_index's device path against its host path."""
import ctypes as C
import os

import numpy as np
import pytest

import fasta_cases as fc
from golden_io import GOLD

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFFFFFFFFFF
GUARD = 64
UNITS = dict(pac=1, rpac=1, text=4, rtext=4, rec=16, blk=16)      # bytes per unit of capacity
WANTED = dict(pac="pac_wanted", rpac="rpac_wanted", text="text_wanted", rtext="rtext_wanted", rec="kept", blk="blocks")
WRITTEN = dict(pac="pac_written", rpac="rpac_written", text="text_written", rtext="rtext_written", rec="rec_written",
               blk="blk_written")


def want_of(data):
    """The host's answer in the device's layouts, and the capacities that hold it exactly."""
    h = fc.host(data)
    codes, rec, blk, total = fc.rule(data)
    assert np.array_equal(codes, h["codes"]) and total == h["total"]
    h.update(rec=rec, blk=blk)
    h["caps"] = dict(pac=len(h["pac"]), rpac=len(h["rpac"]), text=len(h["text"]), rtext=len(h["rtext"]), rec=len(rec),
                     blk=len(blk))
    return h


def run(data, caps, shift=0):
    """One hsa_fasta_device call on `data` placed `shift` bytes into a device buffer (the
    bytes around it '>', which a kernel that read them would count); every output holds its
    capacity and GUARD bytes of 0xA5 behind it.  Returns the raw buffers, the counters by
    name and the return value."""
    import torch
    from hsa_amd import _lib, fasta
    buf = np.full(len(data) + 48, ord(">"), np.uint8)
    buf[shift:shift + len(data)] = np.frombuffer(data, np.uint8)
    d_in = torch.from_numpy(buf).cuda()
    out = {k: torch.full((caps[k] * UNITS[k] + GUARD + 3 & ~3,), 0xA5, dtype=torch.uint8, device="cuda") for k in UNITS}
    ctr = torch.zeros(len(_lib.FA_COUNTERS), dtype=torch.int64, device="cuda")
    scratch = torch.empty(fasta.scratch_bytes(len(data)), dtype=torch.uint8, device="cuda")
    b = _lib.FastaBatch(d_in=d_in.data_ptr() + shift, n_in=len(data), d_counters=ctr.data_ptr(),
                        d_scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
    for k in UNITS:
        setattr(b, "d_" + k, out[k].data_ptr())
        setattr(b, k + "_cap", caps[k])
    rc = _lib.lib().hsa_fasta_device(0, C.byref(b), None)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, fasta.counters(ctr), rc


def check(data, w=None, shift=0):
    """The call on `data` with exact capacities leaves what the host functions make."""
    from hsa_amd import fasta, index_build
    w = w or want_of(data)
    got, c, rc = run(data, w["caps"], shift)
    assert rc == 0
    assert c["refused"] == ONES
    assert (c["seen"], c["kept"], c["blocks"], c["characters"], c["total"], c["T"], c["rev_T"]) == \
        (w["records"], len(w["rec"]), len(w["blk"]), len(w["codes"]), w["total"], w["T"], w["rT"])
    for k in UNITS:
        assert c[WANTED[k]] == c[WRITTEN[k]] == w["caps"][k], k
        n = w["caps"][k] * UNITS[k]
        assert np.array_equal(got[k][:n], np.ascontiguousarray(w[k]).view(np.uint8).reshape(-1)), k
        assert (got[k][n:n + GUARD] == 0xA5).all(), k
    rec = got["rec"][:16 * len(w["rec"])].view(np.uint32).reshape(-1, 4)
    blk = got["blk"][:16 * len(w["blk"])].view(np.uint32).reshape(-1, 4)
    assert index_build.ann_text(fasta.ann_rows(data, rec, blk), c["total"]) == w["ann_text"]
    return got, c


@pytest.mark.parametrize("name", ["tiny", "rep", "nrun"])
def test_fixture_genomes_match_the_committed_files(tmp_path, name):
    from test_index_build import fasta as make_fasta
    data = open(make_fasta(name, str(tmp_path / f"{name}.fa")), "rb").read()
    w = want_of(data)
    got, c = check(data, w)
    pre = os.path.join(GOLD, "index", f"{name}.fa.index")
    assert got["pac"][:c["pac_wanted"]].tobytes() == open(pre + ".pac", "rb").read()
    assert got["rpac"][:c["rpac_wanted"]].tobytes() == open(pre + ".rev.pac", "rb").read()
    assert w["ann_text"] == open(pre + ".ann").read()


def test_edge_records():
    data = fc.edge_fasta()
    w = want_of(data)
    names = [n for n, _ in w["ann"]]
    assert "r74" not in names and "header_only" not in names and {"r75", "r76", "tab", "space", "n" * 256} <= set(names)
    (all_n,) = [b for n, b in w["ann"] if n == "all_n"]
    assert len(all_n) == 1 and all_n[0][1] == all_n[0][0] - 1 and all_n[0][2] == 80
    check(data, w)
    for q in fc.quirk_fastas():
        check(q)


@pytest.mark.parametrize("i", range(10))
def test_length_quirks(i):
    """total % 4 = 0..3, T % 16 == 0 and != 0: both text lengths and both texts are pac_text
    of the host's files."""
    data = fc.length_fastas()[i]
    w = want_of(data)
    _, c = check(data, w)
    assert (c["T"], c["rev_T"]) == (w["T"], w["rT"])


def test_length_cases_cover_every_residue():
    ws = [fc.host(d) for d in fc.length_fastas()]
    assert {w["total"] % 4 for w in ws} == {0, 1, 2, 3}
    assert {w["T"] % 16 == 0 for w in ws} == {True, False}
    assert any(w["T"] < len(w["codes"]) for w in ws) and any(w["rT"] < w["T"] for w in ws)


@pytest.mark.parametrize("i", range(7))
def test_tile_edges_under_every_placement(i):
    data = fc.tile_fastas()[i]
    w = want_of(data)
    for shift in range(16):
        check(data, w, shift)


def test_tile_cases_sit_on_the_edges():
    t = fc.tile_fastas()
    assert t[1][fc.TILE - 1:fc.TILE] == b">" and t[2][fc.TILE - 10:fc.TILE - 9] == b">" and b"\n" not in t[2][fc.TILE - 10:fc.TILE + 1]
    assert t[3][2 * fc.TILE - 4:2 * fc.TILE + 6] == b"N" * 10 and t[4][fc.TILE - 5:fc.TILE + 4] == b"N" * 9
    assert len(t[0]) > 3 * fc.TILE


@pytest.mark.parametrize("part", range(4))
def test_random_inputs(part):
    for seed in range(50 * part, 50 * part + 50):
        check(fc.random_fasta(seed), shift=seed % 16)


@pytest.mark.parametrize("data, off", [(b">a\n" + fc.bases(80) + b"\n>b x>y\n" + fc.bases(80) + b"\n", 88),
                                       (b">a\n" + fc.bases(80) + b"\n>b", 84),
                                       (b"\n>a\n" + fc.bases(80) + b"\n", 0)])
def test_refused_inputs(tmp_path, data, off):
    from hsa_amd import index_build
    assert fc.refused_offset(data) == off
    caps = dict(pac=64, rpac=64, text=32, rtext=32, rec=4, blk=4)
    _, c, rc = run(data, caps)
    assert rc == 0 and c["refused"] == off
    fa = tmp_path / "bad.fa"
    fa.write_bytes(data)
    with pytest.raises(ValueError, match=str(off)):
        index_build.build_index(str(fa))


def test_short_capacities_guards_and_a_second_run():
    data = fc.edge_fasta() + b"\n" + fc.tile_fastas()[3]
    w = want_of(data)
    for k in UNITS:
        caps = dict(w["caps"])
        caps[k] -= 1
        got, c, rc = run(data, caps)
        assert rc == 0 and c[WANTED[k]] == w["caps"][k] and c[WRITTEN[k]] == caps[k], k
        for o in UNITS:
            n = caps[o] * UNITS[o]
            assert (got[o][n:n + GUARD] == 0xA5).all(), (k, o)
            if not (k == "text" and o in ("rtext", "rpac")):      # (a cut forward text spoils the reversed one)
                assert np.array_equal(got[o][:n], np.ascontiguousarray(w[o]).view(np.uint8).reshape(-1)[:n]), (k, o)
        wanted = {o: c[WANTED[o]] for o in UNITS}
        assert wanted == w["caps"]
    a, ca = check(data, w)
    b, cb = check(data, w)
    assert ca == cb and all(np.array_equal(a[k], b[k]) for k in UNITS)


def test_bad_arguments():
    import torch
    from hsa_amd import _lib
    L = _lib.lib()
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    full = dict(d_in=t.data_ptr(), n_in=16, d_pac=t.data_ptr(), pac_cap=8, d_rpac=t.data_ptr(), rpac_cap=8,
                d_text=t.data_ptr(), text_cap=8, d_rtext=t.data_ptr(), rtext_cap=8, d_rec=t.data_ptr(), rec_cap=1,
                d_blk=t.data_ptr(), blk_cap=1, d_counters=t.data_ptr(), d_scratch=t.data_ptr(), scratch_bytes=4096)
    for k in ("d_in", "d_pac", "d_rpac", "d_text", "d_rtext", "d_rec", "d_blk", "d_counters", "d_scratch"):
        assert L.hsa_fasta_device(0, C.byref(_lib.FastaBatch(**dict(full, **{k: None}))), None) == -2, k
        assert b"null" in L.hsa_last_error()
    assert L.hsa_fasta_device(0, None, None) == -2
    assert L.hsa_fasta_device(0, C.byref(_lib.FastaBatch(**dict(full, n_in=(1 << 32) - 256))), None) == -2
    assert L.hsa_fasta_device(0, C.byref(_lib.FastaBatch(**dict(full, scratch_bytes=16))), None) == -2
    assert b"scratch" in L.hsa_last_error()
    assert L.hsa_bwt_files_device(0, 16, None, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 4096, None) == -2
    assert L.hsa_bwt_files_device(0, 0, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 4096, None) == -2


@pytest.mark.parametrize("T", [1, 255, 256, 257, 511, 512, 65535, 65536, 65537, 131073])
def test_bwt_file_bodies(T):
    """Odd and even sample counts, one and two major samples: the code words and both Occ
    arrays equal pack_codes_msb and occ_files.  The words behind the text hold other bits,
    which the call must not count."""
    import torch
    from hsa_amd import fasta, index_io
    codes = np.random.default_rng(T).integers(0, 4, T).astype(np.uint8)
    lsb = index_io.pack_lsb_u32(np.concatenate([codes, np.full((16 - T % 16) % 16 + 32, 3, np.uint8)]))
    msb, minor, major = fasta.bwt_files_device(torch.from_numpy(lsb.view(np.int32)).cuda(), T)
    e_minor, e_major = index_io.occ_files(codes)
    assert np.array_equal(msb.cpu().numpy().view(np.uint32), index_io.pack_codes_msb(codes))
    assert np.array_equal(minor.cpu().numpy().view(np.uint32), e_minor)
    assert np.array_equal(major.cpu().numpy().view(np.uint32), e_major)


def test_host_path_equals_device_path(tmp_path):
    from test_index_build import fasta as make_fasta
    from hsa_amd import index_build
    fa = make_fasta("nrun", str(tmp_path / "nrun.fa"))
    a = index_build.build_index(fa, str(tmp_path / "host"), host=True)
    b = index_build.build_index(fa, str(tmp_path / "dev"))
    assert a == b
    for e in ("pac", "ann", "rev.pac", "bwt", "fmv", "rev.bwt", "rev.fmv", "sa"):
        assert open(tmp_path / f"host.index.{e}", "rb").read() == open(tmp_path / f"dev.index.{e}", "rb").read(), e
