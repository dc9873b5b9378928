// signbytes_host.cpp -- stand-alone test program (g++, also with -fsanitize=address,undefined): the bit logic of k_count_bytes,
// csrc/mc_signbytes.h, compiled for the host from the very header the kernel includes, against the two kernels it replaces on its path:
// the sign words as k_bits_transpose regroups them from bits8[y][x/8][z], and segment_mask on those words the way k_compact
// walks them (a flat plane of ny * nxw words, the word after a segment = the next word of the plane).  A "wavefront" here is a loop
// over 64 lanes that loads what the kernel's lanes load (same offsets, same guards); its masks, the per-block and per-quarter counts,
// the case-13 counts and the validity bits must equal the reference's, bit for bit.  tests/test_signbytes_host.py builds and runs it.
// The header takes its qualifiers from its includer -- <hip/hip_runtime.h> in the product; a host compiler gets them HERE:
#define __device__
#define __forceinline__ inline
#include "../../sdfkit_amd/csrc/mc_signbytes.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sdfk;

static long g_checks = 0, g_fail = 0;
#define CHECK(cond, ...)                                                             \
    do {                                                                             \
        g_checks++;                                                                  \
        if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } \
    } while (0)

struct Grid {
    int nx, ny, nz, nx8, nxw, pitch8, ncx, ncy, ncz, nseg, bpl, nsegp, nchunk;
    Grid(int x, int y, int z) : nx(x), ny(y), nz(z)
    {
        nx8 = (nx + 7) / 8; nxw = (nx + 63) / 64; pitch8 = (nz + 3) & ~3;
        ncx = nx - 1; ncy = ny - 1; ncz = nz - 1; nseg = ncy * nxw; bpl = (nseg + 1023) / 1024; nsegp = (nseg + 7) & ~7; nchunk = (ncz + 511) / 512;
    }
    size_t nbytes() const { return (size_t)ny * nx8 * pitch8; }
};

struct Result {
    std::vector<uint64_t> mask, m13;      // [layer][segment]
    std::vector<uint64_t> blockcnt;       // [layer * bpl + part]: cells | case 13 << 32
    std::vector<uint32_t> wavecnt;        // [(layer * bpl + part) * 4 + quarter]
    std::vector<uint64_t> valid;          // [(chunk * 8 + z % 8) * nsegp + segment], bit (z % 512) / 8
    void init(const Grid& g)
    {
        mask.assign((size_t)g.ncz * g.nseg, 0); m13 = mask;
        blockcnt.assign((size_t)g.ncz * g.bpl, 0); wavecnt.assign((size_t)g.ncz * g.bpl * 4, 0);
        valid.assign((size_t)g.nchunk * 8 * g.nsegp, 0);
    }
};

// k_bits_transpose + k_compact
static void reference(const Grid& g, const std::vector<uint8_t>& b8, std::vector<uint64_t>& words, Result& R)
{
    words.assign((size_t)g.nz * g.ny * g.nxw + 8, 0x5a5a5a5a5a5a5a5aull);   // (the padding k_compact may read holds anything)
    for (int z = 0; z < g.nz; z++)
        for (int y = 0; y < g.ny; y++)
            for (int xw = 0; xw < g.nxw; xw++) {
                uint64_t w = 0;
                for (int b = 0; b < 8; b++)
                    if (xw * 8 + b < g.nx8) w |= (uint64_t)b8[((size_t)y * g.nx8 + xw * 8 + b) * g.pitch8 + z] << (8 * b);
                words[((size_t)z * g.ny + y) * g.nxw + xw] = w;
            }
    R.init(g);
    const size_t plane = (size_t)g.ny * g.nxw;
    for (int z = 0; z < g.ncz; z++)
        for (int i = 0; i < g.nseg; i++) {
            const int xw = i % g.nxw;
            const uint64_t* f = &words[(size_t)z * plane + i];
            uint64_t q13;
            const uint64_t q = segment_mask(f[0], f[1], f[g.nxw], f[g.nxw + 1], f[plane], f[plane + 1], f[plane + g.nxw], f[plane + g.nxw + 1], g.ncx - xw * 64, q13);
            R.mask[(size_t)z * g.nseg + i] = q; R.m13[(size_t)z * g.nseg + i] = q13;
            const uint32_t c = (uint32_t)__builtin_popcountll(q), c13 = (uint32_t)__builtin_popcountll(q13);
            R.blockcnt[(size_t)z * g.bpl + (i >> 10)] += (uint64_t)c | ((uint64_t)c13 << 32);
            R.wavecnt[(size_t)z * g.bpl * 4 + (i >> 8)] += c;
            if (q) R.valid[((size_t)(z >> 9) * 8 + (z & 7)) * g.nsegp + i] |= 1ull << ((z & 511) >> 3);
        }
}

// k_count_bytes, lane by lane
static void by_bytes(const Grid& g, const std::vector<uint8_t>& b8, const std::vector<uint64_t>& words, Result& R)
{
    R.init(g);
    for (int chunk = 0; chunk < g.nchunk; chunk++)
        for (int y = 0; y < g.ncy; y++)
            for (int xw = 0; xw < g.nxw; xw++) {
                const int zc = chunk * 512, i = y * g.nxw + xw;
                // (lanes whose planes all lie beyond the rows load nothing and own no layer: one of them is enough here)
                const int nlanes = g.pitch8 - zc >= 512 ? 64 : (g.pitch8 - zc) / 8 + 1;
                static uint64_t rows[65][2][9];
                memset(rows, 0, sizeof rows);
                uint64_t edge_w[2] = {0, 0}, edge_n[2] = {0, 0};
                for (int lane = 0; lane < nlanes; lane++)
                    for (int v = 0; v < 2; v++)
                        for (int t = 0; t < 9; t++) {
                            const int x8 = 8 * xw + t, z = zc + 8 * lane;
                            rows[lane][v][t] = 0;
                            if (x8 < g.nx8 && z < g.pitch8) memcpy(&rows[lane][v][t], &b8[((size_t)(y + v) * g.nx8 + x8) * g.pitch8 + z], 8);
                        }
                for (int v = 0; v < 2; v++)
                    for (int t = 0; t < 9; t++)
                        if (8 * xw + t < g.nx8 && zc + 512 < g.nz) {
                            const uint64_t e = b8[((size_t)(y + v) * g.nx8 + 8 * xw + t) * g.pitch8 + zc + 512];
                            if (t < 8) edge_w[v] |= e << (8 * t); else edge_n[v] = e & 1;
                        }
                uint64_t w8[64][2], n8[64][2];
                for (int lane = 0; lane < nlanes; lane++)
                    for (int v = 0; v < 2; v++) {
                        if (lane == 63) { w8[lane][v] = edge_w[v]; n8[lane][v] = edge_n[v]; continue; }
                        uint64_t w = 0;
                        for (int t = 0; t < 8; t++) w |= (rows[lane + 1][v][t] & 0xffull) << (8 * t);
                        w8[lane][v] = w; n8[lane][v] = rows[lane + 1][v][8] & 1ull;
                    }
                for (int lane = 0; lane < nlanes; lane++) {
                    const int z = zc + 8 * lane;
                    uint64_t m[8], m13[8];
                    signbytes_lane_masks(rows[lane], w8[lane], n8[lane], g.ncx - xw * 64, g.ncz - z, m, m13);
                    for (int j = 0; j < 8; j++) {
                        if (z + j < g.nz)   // the transposed words themselves (rows[lane] was transposed in place)
                            for (int v = 0; v < 2; v++)
                                CHECK(rows[lane][v][j] == words[((size_t)(z + j) * g.ny + y + v) * g.nxw + xw], "word nx=%d ny=%d nz=%d y=%d xw=%d z=%d", g.nx, g.ny, g.nz, y + v, xw, z + j);
                        if (z + j >= g.ncz) { CHECK(m[j] == 0 && m13[j] == 0, "mask beyond the last layer z=%d", z + j); continue; }
                        R.mask[(size_t)(z + j) * g.nseg + i] = m[j]; R.m13[(size_t)(z + j) * g.nseg + i] = m13[j];
                        const uint32_t c = (uint32_t)__builtin_popcountll(m[j]), c13 = (uint32_t)__builtin_popcountll(m13[j]);
                        R.blockcnt[(size_t)(z + j) * g.bpl + (i >> 10)] += (uint64_t)c | ((uint64_t)c13 << 32);
                        R.wavecnt[(size_t)(z + j) * g.bpl * 4 + (i >> 8)] += c;
                        if (m[j]) R.valid[((size_t)chunk * 8 + j) * g.nsegp + i] |= 1ull << lane;   // (the ballot: bit = lane)
                    }
                }
            }
}

static void run(const Grid& g, const std::vector<uint8_t>& b8, const char* what)
{
    std::vector<uint64_t> words;
    Result A, B;
    reference(g, b8, words, A);
    by_bytes(g, b8, words, B);
    CHECK(A.mask == B.mask, "masks: %s nx=%d ny=%d nz=%d", what, g.nx, g.ny, g.nz);
    CHECK(A.m13 == B.m13, "case-13 masks: %s nx=%d ny=%d nz=%d", what, g.nx, g.ny, g.nz);
    CHECK(A.blockcnt == B.blockcnt, "block counts: %s nx=%d ny=%d nz=%d", what, g.nx, g.ny, g.nz);
    CHECK(A.wavecnt == B.wavecnt, "quarter counts: %s nx=%d ny=%d nz=%d", what, g.nx, g.ny, g.nz);
    CHECK(A.valid == B.valid, "validity bits: %s nx=%d ny=%d nz=%d", what, g.nx, g.ny, g.nz);
}

// sign bytes of a volume given bit by bit; bits beyond nx in the last byte of a row and bytes beyond nz stay as `pad`
template <class F>
static std::vector<uint8_t> fill(const Grid& g, uint8_t pad, F bit)
{
    std::vector<uint8_t> b(g.nbytes(), 0);
    for (int y = 0; y < g.ny; y++)
        for (int x8 = 0; x8 < g.nx8; x8++)
            for (int z = 0; z < g.pitch8; z++) {
                uint8_t v = 0;
                for (int k = 0; k < 8; k++)
                    if (x8 * 8 + k < g.nx && bit(x8 * 8 + k, y, z)) v |= (uint8_t)(1u << k);
                b[((size_t)y * g.nx8 + x8) * g.pitch8 + z] = z < g.nz ? v : pad;
            }
    return b;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

int main()
{
    {   // the transposition on its own: byte j of row i <-> byte i of row j
        uint64_t r[8], s[8];
        for (int rep = 0; rep < 1000; rep++) {
            for (int i = 0; i < 8; i++) s[i] = r[i] = ((uint64_t)rnd() << 32) | rnd();
            signbytes_transpose8(r);
            for (int i = 0; i < 8; i++)
                for (int j = 0; j < 8; j++) CHECK(((r[j] >> (8 * i)) & 0xff) == ((s[i] >> (8 * j)) & 0xff), "transpose8 i=%d j=%d", i, j);
            CHECK(signbytes_next(s[0], 3) == ((s[0] >> 24) & 1), "signbytes_next");
        }
    }
    const int nxs[4] = {64, 65, 72, 128}, nys[2] = {2, 3};
    for (int nx : nxs)
        for (int ny : nys) {
            // nz = 22: three lanes, two padding bytes per row; nz = 528: the 512-layer chunk boundary is crossed (edge bytes), pitch % 8 == 0
            for (int nz : {22, 528}) {
                const Grid g(nx, ny, nz);
                if (g.pitch8 % 8) { printf("bad test extent\n"); return 2; }
                run(g, fill(g, 0x00, [](int, int, int) { return false; }), "all zero");
                run(g, fill(g, 0xff, [](int, int, int) { return true; }), "all one");
                run(g, fill(g, 0xff, [](int x, int y, int z) { return ((x + y + z) & 1) != 0; }), "checkerboard");
                run(g, fill(g, 0x00, [](int x, int y, int z) { return ((x + y + z) & 1) == 0; }), "checkerboard, other parity");
                run(g, fill(g, 0xa5, [](int x, int y, int z) { return (((x >> 1) + y + (z >> 1)) & 1) != 0; }), "checkerboard of 2 x 1 x 2");
                run(g, fill(g, 0x5a, [](int x, int y, int z) { return ((x + z) & 1) != 0 && (y & 1) == 0; }), "stripes (case 13 candidates)");
                for (int density : {2, 16, 128, 240}) {
                    run(g, fill(g, (uint8_t)rnd(), [density](int, int, int) { return (int)(rnd() & 255) < density; }), "random");
                }
            }
            // a single set bit (and a single clear bit) at every byte and bit position of the array
            const Grid g(nx, ny, 14);
            std::vector<uint8_t> zero(g.nbytes(), 0), one(g.nbytes(), 0xff);
            for (size_t p = 0; p < g.nbytes(); p++)
                for (int k = 0; k < 8; k++) {
                    zero[p] = (uint8_t)(1u << k); run(g, zero, "single set bit"); zero[p] = 0;
                    one[p] = (uint8_t)~(1u << k); run(g, one, "single clear bit"); one[p] = 0xff;
                }
        }
    {   // more than 256 and more than 1024 segments: quarters and block parts beyond the first
        const Grid g(130, 400, 14);
        run(g, fill(g, 0x00, [](int, int, int) { return (rnd() & 7) == 0; }), "random, many segments");
    }
    printf("signbytes_host: %ld checks, %ld failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
