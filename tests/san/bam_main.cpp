// The serial core of the BAM loader (hsa_amd/csrc/hsa_bam.h) as plain host C++, for a run under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_bam_san.py): the hop check, the
// field offsets and the per-position decode the kernels run, in a byte loop.
//
//   bam_main <cases.bin> <out.bin>
// cases.bin: per case u32 n, u32 which, i32 trim_qual, then the n bytes of a BAM text from a
// record start on.  out.bin: per case u32 end (1: the end of the text, 2: a truncated or
// inconsistent record), u32 consumed, u32 filtered, u32 reads, then per read u32 name length,
// the name, u32 l_seq, u32 the trimmed length, the l_seq codes, the l_seq qualities.  The
// text is a heap block of exactly n bytes, so a read outside it is a report.
#include <stdio.h>
#include <stdlib.h>

#include "../../hsa_amd/csrc/hsa_bam.h"

struct HeapBytes {
    const uint8_t *p;
    uint32_t operator()(uint64_t o) const { return p[o]; }
};

static void put32(FILE *g, uint32_t v) { fwrite(&v, 4, 1, g); }

// bwa_trim_read (bwaseqio.c:92-103) over the read in its own orientation
static uint32_t trim(const HeapBytes &get, const BamRec &r, int trim_qual)
{
    int s = 0, best = 0;
    uint32_t best_l = r.l_seq;
    if (trim_qual < 1) return r.l_seq;
    for (int64_t l = (int64_t)r.l_seq - 1; l >= 35; --l) {
        s += trim_qual - ((int)bam_qual33(get(bam_qual_at(r, (uint32_t)l))) - 33);
        if (s < 0) break;
        if (s > best) { best = s; best_l = (uint32_t)l; }
    }
    return best_l;
}

static void run_case(const uint8_t *text, uint32_t n, uint32_t which, int trim_qual, FILE *g)
{
    const HeapBytes get{text};
    // first the walk alone, as k_bam_walk counts: records, reads, where and how it ends
    uint64_t pos = 0;
    uint32_t end = 1, filtered = 0, reads = 0;
    while (pos < n) {
        BamRec r;
        if (bam_hop(get, pos, n, r) != BAM_HOP_OK) { end = 2; break; }
        if (bam_selected(which, r.flag) && r.l_seq != 0u) ++reads; else ++filtered;
        if (r.end < pos + 37u || r.end > n) abort();       // what a hop promises
        pos = r.end;
    }
    put32(g, end); put32(g, (uint32_t)pos); put32(g, filtered); put32(g, reads);
    // then the records
    const uint64_t stop = pos;
    for (pos = 0; pos < stop;) {
        BamRec r;
        if (bam_hop(get, pos, n, r) != BAM_HOP_OK) abort();
        pos = r.end;
        if (!bam_selected(which, r.flag) || r.l_seq == 0u) continue;
        uint32_t name_len = 0;
        while (name_len < r.l_read_name && get(r.name + name_len) != 0u) ++name_len;
        put32(g, name_len);
        for (uint32_t i = 0; i < name_len; ++i) fputc((int)get(r.name + i), g);
        put32(g, r.l_seq); put32(g, trim(get, r, trim_qual));
        for (uint32_t p = 0; p < r.l_seq; ++p) fputc((int)bam_code(r, p, get(bam_code_at(r, p))), g);
        for (uint32_t p = 0; p < r.l_seq; ++p) fputc((int)bam_qual33(get(bam_qual_at(r, p))), g);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t head[3];
    int cases = 0;
    while (fread(head, 4, 3, f) == 3) {
        uint8_t *buf = (uint8_t *)malloc(head[0] ? head[0] : 1);
        if (!buf || fread(buf, 1, head[0], f) != head[0]) return 3;
        // (exact size: an empty text gets a 1-byte block the core must not touch either)
        run_case(head[0] ? buf : buf + 1, head[0], head[1], (int)head[2], g);
        free(buf);
        ++cases;
    }
    fclose(f);
    if (fclose(g)) return 3;
    fprintf(stderr, "bam_main: %d cases\n", cases);
    return 0;
}
