/*
 * ref_refine -- drives the COMPILED REFERENCE's bwa_refine_gapped (bwtse.c:536) on
 * fabricated rows.  Test infrastructure only, ours, in the manner of ref_probe.c: it
 * includes the reference's headers, links libhsaref.a, calls the function and restates
 * nothing of it.  It is never linked into, loaded by, or called from the product library.
 *
 *   ref_refine <cases.bin> <out.bin>
 *
 * cases.bin (little-endian):
 *   u32 'HSRC', u32 T, u32 n
 *   n x { u32 len, u32 strand, u32 pos, u32 ori, u32 gap }
 *   T bytes: the text's codes 0..3
 *   sum(len) bytes: the reads' codes 0..4, forward, case after case
 * The text is packed the way the reference reads it (bwtse.c:394:
 * packedDNA[k>>4] >> ((~k&15)<<1) & 3); of the HSP only packedDNA and dnaLength are set,
 * which is all bwa_refine_gapped uses.  Every case is one bwa_seq_t: type unique, len ==
 * full_len, seq and rseq (the reverse complement, codes >= 4 kept), n_gapo = gap ? 1 : 0,
 * n_gape = gap ? gap - 1 : 0, start = 0, end = len - 1, n_multi = 0, occ_pos = pos,
 * ori_pos = ori.  One bwa_refine_gapped call answers the batch.
 *
 * out.bin:
 *   u32 'HSRA', u32 n
 *   n x { u32 occ_pos, ori_pos, start, end, nm, n_cigar, md_len }
 *   sum(n_cigar) u32: the CIGAR words (bwa_cigar_t), case after case; a row without a gap
 *     has none (the reference keeps no CIGAR for it and prints `len`M, bwtse.c:713)
 *   sum(md_len) bytes: the MD strings
 * The file is written only after every case is answered; a case the call leaves without
 * an MD string, or with a start / end outside the read, ends the program with status 2.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "bwtaln.h"
#include "bwtse.h"
#include "HSP.h"

#define CASE_WORDS 5
#define HEAD_WORDS 7

static void die(const char *what, const char *arg)
{
    fprintf(stderr, "ref_refine: %s %s\n", what, arg);
    exit(1);
}

static void *slurp(const char *fn, size_t *sz)
{
    FILE *f = fopen(fn, "rb");
    if (!f) die("cannot open", fn);
    fseek(f, 0, SEEK_END); *sz = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
    void *p = malloc(*sz ? *sz : 1);
    if (*sz && fread(p, 1, *sz, f) != *sz) die("short read of", fn);
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: ref_refine cases.bin out.bin\n"); return 1; }
    size_t sz;
    uint8_t *buf = (uint8_t *)slurp(argv[1], &sz);
    uint32_t hd[3];
    if (sz < sizeof hd) die("no header in", argv[1]);
    memcpy(hd, buf, sizeof hd);
    const uint32_t T = hd[1], n = hd[2];
    if (hd[0] != 0x43525348u) die("not a case file:", argv[1]);            /* 'HSRC' */
    const size_t table = sizeof hd + (size_t)n * CASE_WORDS * 4u;
    if (sz < table + T) die("truncated:", argv[1]);
    uint32_t *cs = (uint32_t *)malloc((size_t)(n ? n : 1) * CASE_WORDS * 4u);
    memcpy(cs, buf + sizeof hd, (size_t)n * CASE_WORDS * 4u);
    const uint8_t *text = buf + table, *reads = text + T;
    size_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t *c = cs + (size_t)i * CASE_WORDS;
        if (c[0] == 0 || c[0] >= (1u << 19) || c[1] > 1 || c[2] >= T || c[4] > 255) die("bad case in", argv[1]);
        if (c[4] == 0 && (uint64_t)c[2] + c[0] > T) die("an ungapped case runs past the text in", argv[1]);
        total += c[0];
    }
    if (sz != table + T + total) die("size does not match the table:", argv[1]);

    HSP hsp;
    memset(&hsp, 0, sizeof hsp);
    hsp.dnaLength = T;
    hsp.packedDNA = (unsigned int *)calloc((size_t)T / 16u + 2u, sizeof(unsigned int));
    for (uint32_t k = 0; k < T; ++k) {
        if (text[k] > 3) die("a text code above 3 in", argv[1]);
        hsp.packedDNA[k >> 4] |= (unsigned int)text[k] << ((~k & 15u) << 1);
    }

    bwa_seq_t *seqs = (bwa_seq_t *)calloc(n ? n : 1, sizeof(bwa_seq_t));
    size_t off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t *c = cs + (size_t)i * CASE_WORDS;
        const uint32_t len = c[0], gap = c[4];
        bwa_seq_t *s = seqs + i;
        s->seq = (ubyte_t *)malloc(len);
        s->rseq = (ubyte_t *)malloc(len);
        for (uint32_t y = 0; y < len; ++y) {
            const uint8_t v = reads[off + y];
            s->seq[y] = v;
            s->rseq[len - 1u - y] = v < 4 ? (ubyte_t)(3 - v) : v;
        }
        off += len;
        s->type = BWA_TYPE_UNIQUE;
        s->len = len; s->full_len = len;
        s->strand = c[1];
        s->occ_pos = c[2]; s->ori_pos = c[3];
        s->n_gapo = gap ? 1 : 0;
        s->n_gape = gap ? gap - 1 : 0;
        s->start = 0; s->end = (int)len - 1;
        s->n_multi = 0;
    }

    bwa_refine_gapped(&hsp, (int)n, seqs);

    uint32_t *head = (uint32_t *)calloc((size_t)(n ? n : 1) * HEAD_WORDS, 4);
    size_t n_words = 0, n_md = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const bwa_seq_t *s = seqs + i;
        uint32_t *h = head + (size_t)i * HEAD_WORDS;
        if (!s->md || s->start < 0 || s->end >= (int)s->len || s->n_cigar < 0 || (s->n_cigar > 0 && !s->cigar) ||
            (cs[(size_t)i * CASE_WORDS + 4] != 0) != (s->n_cigar > 0)) {
            fprintf(stderr, "ref_refine: case %u is not answered\n", i);
            return 2;
        }
        h[0] = s->occ_pos; h[1] = s->ori_pos; h[2] = (uint32_t)s->start; h[3] = (uint32_t)s->end;
        h[4] = s->nm; h[5] = (uint32_t)s->n_cigar; h[6] = (uint32_t)strlen(s->md);
        n_words += h[5]; n_md += h[6];
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f) die("cannot write", argv[2]);
    const uint32_t oh[2] = {0x41525348u, n};                                /* 'HSRA' */
    int ok = fwrite(oh, 4, 2, f) == 2 && fwrite(head, 4, (size_t)n * HEAD_WORDS, f) == (size_t)n * HEAD_WORDS;
    for (uint32_t i = 0; i < n && ok; ++i)
        if (seqs[i].n_cigar) ok = fwrite(seqs[i].cigar, 4, (size_t)seqs[i].n_cigar, f) == (size_t)seqs[i].n_cigar;
    for (uint32_t i = 0; i < n && ok; ++i) {
        const size_t l = head[(size_t)i * HEAD_WORDS + 6];
        ok = fwrite(seqs[i].md, 1, l, f) == l;
    }
    if (fclose(f) != 0 || !ok) die("short write of", argv[2]);
    fprintf(stderr, "ref_refine: %u cases, %zu CIGAR words, %zu MD bytes\n", n, n_words, n_md);

    for (uint32_t i = 0; i < n; ++i) {
        free(seqs[i].seq); free(seqs[i].rseq); free(seqs[i].cigar); free(seqs[i].md);
    }
    free(seqs); free(head); free(hsp.packedDNA); free(cs); free(buf);
    return 0;
}
