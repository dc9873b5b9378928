// lib_redistance.hip -- redistancing of voxel volumes (Voxels.Redistance): a signed distance to the iso-surface of a volume by
// a first-order Eikonal solve (Godunov upwind, Jacobi sweeps to the fixed point: the fast iterative method family).
// Contract: include/sdfkit_hip.h, "Redistancing".  Arithmetic: redistance.h (shared with a host test).
//
// T lives in two f32 buffers in TILE-MAJOR order: the volume is padded to whole 8 x 8 x 8 tiles, the 512 voxels of a tile are
// contiguous (x slowest, z fastest inside the tile), padding voxels hold +inf for ever.  A frozen (front) voxel is stored with
// its sign bit set (T >= 0, so -T0, -0.0 for a zero): no separate mask.
// Schedule: block-active Jacobi.  Sweep k reads buffer (k - 1) & 1 and writes buffer k & 1; every tile has a "changed in sweep
// k" flag (two arrays, alternating); a tile is swept in sweep k only if it or one of its six face neighbours changed in sweep
// k - 1 (a voxel update reads the 6-neighbourhood only, so any other tile could not change: skipping it IS the full Jacobi
// sweep).  A swept tile rewrites all of its 512 voxels, so both buffers agree on every tile that did not change last sweep.
// Fixed point: ctl->last = the last sweep that changed a voxel (atomicMax); a sweep k > last + 1 returns at once, so the host
// queues sweeps in batches and reads `last` once per batch.  Host side: the buffers, the flags and the control block are the
// scratch of a Staged (device_stage.h), which also makes the reads of the control block.
#include "lib_internal.h"
#include "device_stage.h"
#include "device_wave.h"
#include "redistance.h"

namespace {

using namespace sdfk_redistance;

constexpr int kBlock = 256;
constexpr int kTileVox = kTile * kTile * kTile;   // 512: two voxels per lane
constexpr int kHalo = kTile + 2;
constexpr int kBatch = 32;                        // sweeps queued between two reads of ctl->last

struct Ctl {
    int last;                         // last sweep that changed a voxel; 0: the front pass found a front; -1: no front
    unsigned nonfinite;               // k_rd_check
    unsigned long long tile_sweeps;   // tiles swept
    unsigned long long front;         // front voxels
    unsigned long long clamped;       // voxels whose T exceeds the band at the end
};

struct Geo {
    int nx, ny, nz, pitch;            // the volume (rows of `pitch` voxels)
    int tx, ty, tz;                   // tiles
    double h[3];
};

__device__ __forceinline__ size_t tile_base(const Geo& G, int ix, int iy, int iz) { return ((size_t)((size_t)ix * G.ty + iy) * G.tz + iz) * kTileVox; }

// the tile-major slot of voxel (x, y, z) (inside the padded grid)
__device__ __forceinline__ size_t slot_of(const Geo& G, int x, int y, int z)
{
    return tile_base(G, x >> 3, y >> 3, z >> 3) + (size_t)(((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
}

__global__ __launch_bounds__(kBlock) void k_rd_check(const float* __restrict__ v, Geo G, Ctl* __restrict__ ctl)
{
    const int64_t n = (int64_t)G.nx * G.ny * G.nz;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t row = i / G.nz;
        const int k = (int)(i - row * G.nz);
        if (!isfinite(v[(size_t)row * G.pitch + k])) bad = true;
    }
    if (bad) atomicOr(&ctl->nonfinite, 1u);
}

// One block per tile: T0 (and the frozen bit) of its voxels into both buffers, the tile's "changed in sweep 0" flag.
__global__ __launch_bounds__(kBlock) void k_rd_front(const float* __restrict__ v, Geo G, float iso, float* __restrict__ t_a, float* __restrict__ t_b,
                                                     uint32_t* __restrict__ flag0, Ctl* __restrict__ ctl)
{
    const int tile = blockIdx.x;
    const int iz = tile % G.tz, iy = (tile / G.tz) % G.ty, ix = tile / (G.tz * G.ty);
    const size_t base = (size_t)tile * kTileVox;
    const double di = (double)iso;
    int nfront = 0;
    for (int l = threadIdx.x; l < kTileVox; l += kBlock) {
        const int p[3] = {ix * kTile + (l >> 6), iy * kTile + ((l >> 3) & 7), iz * kTile + (l & 7)};
        float t = INFINITY;
        if (p[0] < G.nx && p[1] < G.ny && p[2] < G.nz) {
            const int n[3] = {G.nx, G.ny, G.nz};
            const size_t o = ((size_t)p[0] * G.ny + p[1]) * G.pitch + p[2];
            const size_t stride[3] = {(size_t)G.ny * G.pitch, (size_t)G.pitch, 1};
            const double s = (double)v[o] - di;
            double sn[6];
            bool in[6];
            for (int a = 0; a < 3; a++) {
                in[2 * a] = p[a] > 0;
                in[2 * a + 1] = p[a] + 1 < n[a];
                sn[2 * a] = in[2 * a] ? (double)v[o - stride[a]] - di : 0.0;
                sn[2 * a + 1] = in[2 * a + 1] ? (double)v[o + stride[a]] - di : 0.0;
            }
            float t0;
            if (rd_front(s, sn, in, G.h, &t0)) {
                t = -t0;
                nfront++;
            }
        }
        t_a[base + l] = t;
        t_b[base + l] = t;
    }
    const int total = __syncthreads_count(nfront > 0) ? 1 : 0;
    // (the count itself: one atomic per wave)
    wave_add(&ctl->front, (unsigned long long)nfront);
    if (threadIdx.x == 0) {
        flag0[tile] = (uint32_t)total;
        if (total) atomicMax(&ctl->last, 0);
    }
}

__global__ __launch_bounds__(kBlock) void k_rd_sweep(Geo G, float band, int k, const float* __restrict__ t_in, float* __restrict__ t_out,
                                                     const uint32_t* __restrict__ flag_in, uint32_t* __restrict__ flag_out, Ctl* ctl)
{
    __shared__ float s[kHalo][kHalo][kHalo];
    // (atomically updated by the blocks of THIS sweep to k, which keeps the test true)
    if (__atomic_load_n(&ctl->last, __ATOMIC_RELAXED) < k - 1) return;   // the fixed point was reached before this sweep
    const int tile = blockIdx.x;
    const int iz = tile % G.tz, iy = (tile / G.tz) % G.ty, ix = tile / (G.tz * G.ty);
    uint32_t act = flag_in[tile];
    if (ix > 0) act |= flag_in[tile - G.tz * G.ty];
    if (ix + 1 < G.tx) act |= flag_in[tile + G.tz * G.ty];
    if (iy > 0) act |= flag_in[tile - G.tz];
    if (iy + 1 < G.ty) act |= flag_in[tile + G.tz];
    if (iz > 0) act |= flag_in[tile - 1];
    if (iz + 1 < G.tz) act |= flag_in[tile + 1];
    if (!act) {
        if (threadIdx.x == 0) flag_out[tile] = 0;
        return;
    }
    // the tile and its six face halos (edges and corners of the 10^3 box are never read)
    for (int l = threadIdx.x; l < kHalo * kHalo * kHalo; l += kBlock) {
        const int lz = l % kHalo, ly = (l / kHalo) % kHalo, lx = l / (kHalo * kHalo);
        const int outx = (lx == 0 || lx == kHalo - 1), outy = (ly == 0 || ly == kHalo - 1), outz = (lz == 0 || lz == kHalo - 1);
        if (outx + outy + outz > 1) continue;
        const int x = ix * kTile + lx - 1, y = iy * kTile + ly - 1, z = iz * kTile + lz - 1;
        float t = INFINITY;
        if (x >= 0 && y >= 0 && z >= 0 && x < G.tx * kTile && y < G.ty * kTile && z < G.tz * kTile) t = t_in[slot_of(G, x, y, z)];
        s[lx][ly][lz] = t;
    }
    __syncthreads();
    const size_t base = (size_t)tile * kTileVox;
    int changed = 0;
    for (int l = threadIdx.x; l < kTileVox; l += kBlock) {
        const int lx = (l >> 6) + 1, ly = ((l >> 3) & 7) + 1, lz = (l & 7) + 1;
        const float raw = s[lx][ly][lz];
        float out = raw;
        // frozen voxels (sign bit) keep T0; padding voxels keep +inf
        if (!signbit(raw) && ix * kTile + lx - 1 < G.nx && iy * kTile + ly - 1 < G.ny && iz * kTile + lz - 1 < G.nz) {
            const float tn[6] = {fabsf(s[lx - 1][ly][lz]), fabsf(s[lx + 1][ly][lz]), fabsf(s[lx][ly - 1][lz]),
                                 fabsf(s[lx][ly + 1][lz]), fabsf(s[lx][ly][lz - 1]), fabsf(s[lx][ly][lz + 1])};
            out = rd_sweep_voxel(raw, tn, G.h, band);
            changed |= out < raw ? 1 : 0;
        }
        t_out[base + l] = out;
    }
    changed = __syncthreads_or(changed);
    if (threadIdx.x == 0) {
        flag_out[tile] = changed ? 1u : 0u;
        if (changed) atomicMax(&ctl->last, k);
        atomicAdd(&ctl->tile_sweeps, 1ull);
    }
}

// One lane per voxel, z fastest: the clamp and the input's sign into dst.
__global__ __launch_bounds__(kBlock) void k_rd_finish(const float* __restrict__ src, float* __restrict__ dst, Geo G, float iso, float band,
                                                      const float* __restrict__ t, Ctl* __restrict__ ctl)
{
    const int64_t n = (int64_t)G.nx * G.ny * G.nz;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool over = false;
    if (i < n) {
        const int z = (int)(i % G.nz);
        const int64_t row = i / G.nz;
        const int y = (int)(row % G.ny), x = (int)(row / G.ny);
        const size_t o = (size_t)row * G.pitch + z;
        const float tv = fabsf(t[slot_of(G, x, y, z)]);
        over = tv > band;
        dst[o] = rd_finish(tv, (double)src[o] - (double)iso, band);
    }
    const int c = __syncthreads_count(over);
    if (threadIdx.x == 0 && c) atomicAdd(&ctl->clamped, (unsigned long long)c);
}

bool same_box(const sdfk_volume* a, const sdfk_volume* b)
{
    if (a->nx != b->nx || a->ny != b->ny || a->nz != b->nz || a->nz_global != b->nz_global || a->z0 != b->z0) return false;
    for (int k = 0; k < 3; k++)
        if (a->gmin[k] != b->gmin[k] || a->gmax[k] != b->gmax[k]) return false;
    return true;
}

int redistance(const sdfk_volume* src, sdfk_volume* dst, const float d[3], float iso, float band, int64_t stats[4])
{
    static const char* who = "sdfk_volume_redistance";
    Geo G{};
    G.nx = src->nx; G.ny = src->ny; G.nz = src->nz; G.pitch = src->pitch();
    G.tx = (G.nx + kTile - 1) / kTile; G.ty = (G.ny + kTile - 1) / kTile; G.tz = (G.nz + kTile - 1) / kTile;
    for (int k = 0; k < 3; k++) G.h[k] = (double)d[k];
    const int64_t tiles = (int64_t)G.tx * G.ty * G.tz;
    if (tiles >= (int64_t(1) << 31)) return fail(SDFK_ERR_INVALID, "%s: 2^31 tiles of 8^3 voxels or more", who);
    const int64_t nvox = (int64_t)G.nx * G.ny * G.nz;
    Staged st;
    Ctl* ctl = st.scratch<Ctl>(1);
    Ctl host{};
    // 1. refusal: the finite check, before anything of dst is touched
    {
        ProfScope ps("k_rd_check");
        st.run([&] { return hipMemsetAsync(ctl, 0, sizeof(Ctl), g.stream); });
        st.run([&] { hipLaunchKernelGGL(k_rd_check, dim3((unsigned)grid_for((size_t)nvox, kBlock, 4096)), dim3(kBlock), 0, g.stream, src->values, G, ctl); });
        st.read(&host, ctl, sizeof(Ctl));
    }
    st.run([&] { return host.nonfinite ? fail(SDFK_ERR_INVALID, "%s: the volume holds a NaN or infinite value", who) : (int)SDFK_OK; });
    float* t[2];
    uint32_t* flag[2];
    for (int b = 0; b < 2; b++) {
        t[b] = st.scratch<float>((size_t)tiles * kTileVox);
        flag[b] = st.scratch<uint32_t>((size_t)tiles);
    }
    // 2. front
    {
        ProfScope ps("k_rd_front");
        st.run([&] { return hipMemsetAsync(&ctl->last, 0xff, sizeof(int), g.stream); });   // -1: no front yet
        st.run([&] { hipLaunchKernelGGL(k_rd_front, dim3((unsigned)tiles), dim3(kBlock), 0, g.stream, src->values, G, iso, t[0], t[1], flag[0], ctl); });
    }
    // 3 / 4. sweeps to the fixed point, a batch at a time
    int queued = 0;
    while (st.ok()) {
        st.run([&] {
            ProfScope ps("k_rd_sweep");
            for (int b = 0; b < kBatch; b++) {
                const int k = ++queued;
                hipLaunchKernelGGL(k_rd_sweep, dim3((unsigned)tiles), dim3(kBlock), 0, g.stream, G, band, k, t[(k - 1) & 1], t[k & 1], flag[(k - 1) & 1],
                                   flag[k & 1], ctl);
            }
        });
        st.read(&host, ctl, sizeof(Ctl));
        if (!st.ok() || host.last < queued) break;   // the last queued sweep changed nothing (or never ran)
        st.run([&] { return queued > (1 << 30) ? fail(SDFK_ERR_INVALID, "%s: no fixed point after 2^30 sweeps", who) : (int)SDFK_OK; });
    }
    // 5. result (both buffers agree at the fixed point)
    if (st.ok()) {
        resolve_dependents(dst);   // (a queued mesh may still read the old values)
        volume_values_changed(dst);
        ProfScope ps("k_rd_finish");
        st.run([&] {
            hipLaunchKernelGGL(k_rd_finish, dim3((unsigned)((nvox + kBlock - 1) / kBlock)), dim3(kBlock), 0, g.stream, src->values, dst->values, G, iso, band,
                               t[0], ctl);
        });
        if (dst->colors && dst != src)
            st.run([&] {
                return src->colors ? hipMemcpyAsync(dst->colors, src->colors, src->nalloc() * 3 * sizeof(float), hipMemcpyDeviceToDevice, g.stream)
                                   : hipMemsetAsync(dst->colors, 0, dst->nalloc() * 3 * sizeof(float), g.stream);
            });
        if (stats) st.read(&host, ctl, sizeof(Ctl));
    }
    if (int r = st.finish(who, false)) return r;   // (no wait of its own: with stats the read above was one)
    if (stats) {
        stats[0] = host.last + 1;   // the sweeps of a full Jacobi iteration, the one that changes nothing included (0: no front)
        stats[1] = (int64_t)host.tile_sweeps;
        stats[2] = (int64_t)host.front;
        stats[3] = (int64_t)host.clamped;
    }
    return SDFK_OK;
}

}  // namespace

extern "C" int sdfk_volume_redistance(const sdfk_volume* src, sdfk_volume* dst, float iso_value, float max_distance, int64_t stats[4])
{
    static const char* who = "sdfk_volume_redistance";
    StateScope in_owner_context(src ? src->owner : nullptr);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int r = require_init()) return r;
    if (!src || !dst) return fail(SDFK_ERR_INVALID, "%s: null argument", who);
    if (src->owner != dst->owner) return fail(SDFK_ERR_INVALID, "%s: the volumes belong to different devices", who);
    if (src->elided || !src->values || dst->elided || !dst->values) return fail(SDFK_ERR_INVALID, "%s: a volume has no storage", who);
    if (src->nx < 1 || src->ny < 1 || src->nz < 1) return fail(SDFK_ERR_INVALID, "%s: empty volume", who);
    // a box with max <= min or a NaN / infinite bound on an axis (sdfk_volume_create takes any box): the iteration has no fixed
    // point on a negative cell size, and a negative T would read as frozen.  (Before same_box: a NaN bound equals nothing.)
    float d[3], m[3], outside;
    grid_constants(src, d, m, &outside);
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(d[k]) || !(d[k] > 0.0f))
            return fail(SDFK_ERR_INVALID, "%s: the cell sizes (%g, %g, %g) must be finite and > 0", who, (double)d[0], (double)d[1], (double)d[2]);
    if (!same_box(src, dst)) return fail(SDFK_ERR_INVALID, "%s: dst has another shape or box than src", who);
    if (!std::isfinite(iso_value)) return fail(SDFK_ERR_INVALID, "%s: iso_value must be finite", who);
    if (!(max_distance >= 0.0f)) return fail(SDFK_ERR_INVALID, "%s: max_distance must be >= 0 (+inf: the full field)", who);
    return redistance(src, dst, d, iso_value, max_distance, stats);
}
