// device_forest.h -- the label rounds of a min-hooking forest over "n nodes, parent array": the control block, what a hook kernel
// does with it, the pointer-jumping launch and the host's round driver.  parent[v] <= v always; a unit's hook kernel offers lower
// parents by atomicMin (labels only decrease and always name a node of the same component), and
//   k_forest_shortcut   one lane per node: parent[v] = parent[parent[v]], one jump per launch; changes are counted.  A launch that
//                       finds that the launch before it changed nothing returns at once: the forest is flat.
// The host queues a hook round and kForestShortcuts shortcut launches, reads the control block once, queues more shortcut launches
// while the last one still changed something, and ends when a hook round on a flat forest changed nothing.  Every verdict is read
// from a counter that the launch BEFORE the reader finished: no launch relies on seeing another workgroup's writes, a stale read
// only costs a round.  Both loops are capped: exceeding a cap is a failure, never an endless loop.  Each unit that includes this
// gets its own copy of the kernel.  hipcc only.
#pragma once
#include "lib_internal.h"
#include "device_stage.h"
#include "device_wave.h"

#include <algorithm>

namespace {

constexpr int kForestBlock = 256;
constexpr int kForestShortcuts = 8;          // shortcut launches queued per read of the control block
constexpr int kForestMaxShortcutBatches = 8;   // per hook round: 64 jumps flatten any tree of fewer than 2^31 nodes (depth halves per jump)

struct ForestCtl {
    unsigned count[3];                        // changes of launch q in slot q % 3
    unsigned pad;
    unsigned long long hook_changes;          // over all hook rounds
    unsigned long long rounds, shortcuts;     // hook rounds run, shortcut launches that worked
};

// A hook kernel, launch number q: first this, by every thread ...
__device__ __forceinline__ void forest_hook_begin(ForestCtl* ctl, int q)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->count[(q + 1) % 3] = 0;
        ctl->rounds += 1;
    }
}
// ... and at its end, by every lane of every wave, with the number of parents the lane lowered
__device__ __forceinline__ void forest_hook_end(ForestCtl* ctl, int q, unsigned changed)
{
    const unsigned long long n = wave_sum(changed);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(&ctl->count[q % 3], (unsigned)n);
        atomicAdd(&ctl->hook_changes, n);
    }
}

__global__ __launch_bounds__(kForestBlock) void k_forest_shortcut(int32_t* parent, int64_t n, ForestCtl* ctl, int q)
{
    const unsigned before = ctl->count[(q + 2) % 3];   // (of the launch before this one: complete)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->count[(q + 1) % 3] = 0;
        if (before) ctl->shortcuts += 1;
    }
    if (!before) return;   // flat already: this launch's own count stays 0
    const int64_t v = (int64_t)blockIdx.x * kForestBlock + threadIdx.x;
    unsigned changed = 0;
    if (v < n) {
        const int32_t p = __atomic_load_n(&parent[v], __ATOMIC_RELAXED);
        const int32_t gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
        if (gp < p) {
            __atomic_store_n(&parent[v], gp, __ATOMIC_RELAXED);
            changed = 1;
        }
    }
    const unsigned long long sum = wave_sum(changed);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&ctl->count[q % 3], (unsigned)sum);
}

// The rounds over parent[0 .. n), which the caller has initialised (parent[v] <= v), as steps of `st`; synchronises at every read
// of the control block.  hook(ctl, q) queues one hook round as launch number q -- a kernel that calls forest_hook_begin and
// forest_hook_end -- and returns SDFK_OK or an SDFK_ERR_*.  *host receives the control block as last read (rounds, shortcuts).
// More than max_rounds hook rounds, or shortcut launches that do not flatten the forest, fail through `st` with `who`.
template <class Hook>
inline void forest_rounds(Staged& st, int32_t* parent, int64_t n, ForestCtl* ctl, ForestCtl* host, int64_t max_rounds, const char* who,
                          const char* shortcut_span, Hook&& hook)
{
    *host = ForestCtl{};
    st.run([&] { return hipMemsetAsync(ctl, 0, sizeof(ForestCtl), g.stream); });
    const unsigned grid = (unsigned)std::max<int64_t>(1, (n + kForestBlock - 1) / kForestBlock);
    int q = 0;   // launches numbered so far (only q % 3 is used)
    bool flat = true;
    int batches = 0;
    unsigned long long hook_before = 0;
    while (st.ok()) {
        if (flat) {
            if ((int64_t)host->rounds >= max_rounds) {
                st.run([&] { return fail(SDFK_ERR_INVALID, "%s: the label rounds did not end within %lld", who, (long long)max_rounds); });
                break;
            }
            hook_before = host->hook_changes;
            batches = 0;
            q = (q + 1) % 3;
            st.run([&] { return hook(ctl, q); });
        } else if (++batches > kForestMaxShortcutBatches) {
            st.run([&] { return fail(SDFK_ERR_INVALID, "%s: the shortcut launches did not flatten the labels", who); });
            break;
        }
        st.run([&] {
            ProfScope ps(shortcut_span);
            for (int b = 0; b < kForestShortcuts; b++) {
                q = (q + 1) % 3;
                hipLaunchKernelGGL(k_forest_shortcut, dim3(grid), dim3(kForestBlock), 0, g.stream, parent, n, ctl, q);
            }
        });
        st.read(host, ctl, sizeof(ForestCtl));
        if (!st.ok()) break;
        flat = host->count[q] == 0;                                 // the last shortcut launch changed nothing
        if (flat && host->hook_changes == hook_before) break;       // and the hook round before them, on a flat forest, neither
    }
}

}  // namespace
