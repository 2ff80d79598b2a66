// The serial core of the BGZF inflater (hsa_amd/csrc/hsa_inflate.h) as plain host C++, for a
// run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_inflate_san.py): the
// same bit reader, tables, symbol loop and CRC pieces the kernel runs, with a byte-loop sink.
//
//   inflate_main <cases.bin> <out.bin>
// cases.bin: per case u32 in_len, u32 isize, u32 crc, then the payload.  out.bin: per case
// u32 status, then the isize bytes of the block's slice.  The payload and the slice are heap
// blocks of exactly in_len and isize bytes, so a read or write outside them is a report.
#include <stdio.h>
#include <stdlib.h>

#include "../../hsa_amd/csrc/hsa_inflate.h"

struct ByteSink {
    uint8_t *out;
    uint32_t isize;
    uint32_t pos = 0;
    int literal(uint8_t c)
    {
        if (pos >= isize) return HSA_INF_E_OUTPUT;
        out[pos++] = c;
        return 0;
    }
    int match(uint32_t dist, uint32_t len)
    {
        if (dist > pos) return HSA_INF_E_DIST;
        if (len > isize - pos) return HSA_INF_E_OUTPUT;
        const uint32_t src = pos - dist;
        for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[src + (i < dist ? i : i % dist)];
        pos += len;
        return 0;
    }
};

static uint32_t inflate_block(const uint8_t *payload, uint32_t in_len, uint8_t *out, uint32_t isize, uint32_t crc)
{
    static uint32_t crc_tab[256];
    static InfTables tables;
    for (uint32_t i = 0; i < 256u; ++i) crc_tab[i] = inf_crc_entry(i);
    InfBits bits;
    inf_open(bits, payload, in_len);
    ByteSink sink{out, isize};
    uint32_t st = (uint32_t)inf_stream(bits, tables, sink);
    if (st == HSA_INF_OK && sink.pos != isize) st = HSA_INF_E_SIZE;
    if (st == HSA_INF_OK) {
        uint32_t sum = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) sum ^= inf_crc_term(crc_tab, out, isize, lane, 64u);
        if (~sum != crc) st = HSA_INF_E_CRC;
    }
    return st;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint32_t head[3];
    int n = 0;
    while (fread(head, 4, 3, f) == 3) {
        uint8_t *payload = (uint8_t *)malloc(head[0] ? head[0] : 1);
        uint8_t *out = (uint8_t *)calloc(head[1] ? head[1] : 1, 1);
        if (!payload || !out || fread(payload, 1, head[0], f) != head[0]) return 3;
        // (exact sizes: an empty payload or slice gets a 1-byte block the core must not touch either)
        uint8_t *p = head[0] ? payload : payload + 1, *o = head[1] ? out : out + 1;
        const uint32_t st = inflate_block(p, head[0], o, head[1], head[2]);
        fwrite(&st, 4, 1, g);
        fwrite(out, 1, head[1], g);
        free(payload);
        free(out);
        ++n;
    }
    fclose(f);
    if (fclose(g)) return 3;
    fprintf(stderr, "inflate_main: %d cases\n", n);
    return 0;
}
