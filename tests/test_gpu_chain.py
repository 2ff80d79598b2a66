"""The retry rules of hsa_amd.chain's drivers: search64 runs again with more hit room while
reads are left unfinished, refine64 doubles its strides while a CIGAR or an MD string does
not fit.  Each is started short on purpose and compared with a run that starts with ample
room, on the golden indexes under gapped options (-n 4 -o 1)."""
import numpy as np
import pytest

from golden_io import INDEX
from hsa_amd import index_io
from test_gpu_refine import index_text

pytestmark = pytest.mark.gpu


def gapped_batch(index, n, L, seed, **kw):
    """(the index, the batch dict, the regime, seed_len) of n reads of L bases cut from the
    golden index's text and changed as kw tells synth.make_reads, for a search with -n 4 -o 1."""
    from hsa_amd import chain, synth
    from hsa_amd._lib import pad_codes
    from oracle_ctypes import default_opt
    text = index_io.read_pac(INDEX[index])
    reads, _ = synth.make_reads(text, [(0, len(text))], n, L, seed, **kw)
    od = default_opt()
    od.update(max_diff=4, fnr=-1.0, max_gapo=1)
    od["mode"] &= ~0x01
    b = dict(jobs=chain.to_device(chain.make_jobs(np.full(n, L), od["max_diff"], od["seed_len"])),
             codes=chain.to_device(pad_codes(reads.reshape(-1))), n_jobs=n, max_len=L)
    return index_text(index), b, chain.local_regime(od, L)[2], od["seed_len"]


def hit_lists(t, n):
    """n_aln, flags and each read's records of the search tensors t, on the host."""
    from hsa_amd._lib import ALN64_WORDS
    n_aln, flags, off = t["n_aln"].cpu().numpy(), t["flags"].cpu().numpy(), t["hit_off"].cpu().numpy()
    hits = t["hits"].cpu().numpy().view(np.uint32)[:t["hit_cap"] * ALN64_WORDS].reshape(-1, ALN64_WORDS)
    return n_aln, flags, [hits[int(off[j]):int(off[j]) + max(int(n_aln[j]), 0)] for j in range(n)]


def test_search64_runs_again_with_more_hit_room():
    """On the repeat text a read has up to three records (317 for these 300 reads by the CPU
    restatement), so one record per read cannot hold them."""
    from hsa_amd import chain
    n = 300
    gi, b, rg, seed = gapped_batch("rep", n, 60, 733, max_mm=2)
    ample = chain.search64(gi, b, 0, n, rg, seed)
    short = chain.search64(gi, b, 0, n, rg, seed, hit_cap=n)
    assert ample["hit_cap"] == 64 * n, "the ample run itself ran out of room"
    assert short["hit_cap"] > n and short["hit_cap"] % (8 * n) == 0, "one record per read sufficed: no retry was taken"
    a_n, a_f, a_h = hit_lists(ample, n)
    s_n, s_f, s_h = hit_lists(short, n)
    assert int(a_n.sum()) > n, "the batch has no more records than reads"
    assert np.array_equal(s_n, a_n) and np.array_equal(s_f, a_f)
    bad = [j for j in range(n) if not np.array_equal(s_h[j], a_h[j])]
    assert not bad, f"{len(bad)} reads' hit records differ, first {bad[:5]}"


def test_refine64_doubles_its_strides_until_every_row_fits():
    from hsa_amd import chain
    n = 200
    gi, b, rg, seed = gapped_batch("tiny", n, 100, 43, indel=True, max_mm_indel=1)
    t = dict(b, **chain.hit_positions64(gi, chain.search64(gi, b, 0, n, rg, seed), n, 8))
    ample = chain.refine64(gi, t)
    short = chain.refine64(gi, t, cigar_stride=1, md_stride=4)
    assert (ample["cigar_stride"], ample["md_stride"]) == (16, 128), "the ample run itself doubled"
    assert short["cigar_stride"] >= 2 and short["md_stride"] == 4 * short["cigar_stride"], "no doubling was taken"
    host = lambda o, k, dt, w: o[k].cpu().numpy().view(dt).reshape(-1, w)      # noqa: E731
    m = int(ample["ctr"][0])
    assert m >= n // 2 and int(ample["ctr"][6]) > 0, "no gapped row among the rows"
    assert [int(v) for v in short["ctr"].cpu().numpy()[:7]] == [int(v) for v in ample["ctr"].cpu().numpy()[:7]]
    rows, rows_s = host(ample, "rows", np.uint32, 8)[:m], host(short, "rows", np.uint32, 8)[:m]
    assert np.array_equal(rows_s, rows)
    assert np.array_equal(host(short, "rpos", np.uint64, 2)[:m], host(ample, "rpos", np.uint64, 2)[:m])
    cg, cg_s = host(ample, "cigar", np.uint32, 16), host(short, "cigar", np.uint32, short["cigar_stride"])
    md, md_s = host(ample, "md", np.uint8, 128), host(short, "md", np.uint8, short["md_stride"])
    assert int(rows[:, 1].max()) >= 3, "no row has a gapped CIGAR"
    for r in range(m):
        nc, nm = int(rows[r, 1]), int(rows[r, 3])
        assert np.array_equal(cg_s[r, :nc], cg[r, :nc]) and np.array_equal(md_s[r, :nm], md[r, :nm]), r
