// rm_rows.hip -- rows of a per-node table through a node list
// (part of libradiomedium_hip.so; gfx950 only, -ffp-contract=off, no fast-math; overview at the top of rm_engine.h)
//
// The tables of E11, E13, E14 and E15 are rows of `words` 64-bit words per node index.  A list call moves entry k of a pinned,
// host-mapped block to or from row nodes[k] of such a table, one word per lane with plain 64-bit loads and stores (the store width
// towards host-mapped memory is the one tools/pcie_store_width.hip measured).  `words` is a run-time value: a lane divides once,
// for its first word, and then steps (row, word) by the stride's quotient and remainder -- no division in the loop.
#include "rm_device.hpp"

namespace rm {

// one lane per word, 256-thread workgroups, at most 64 of them: 16 384 lanes per stride
constexpr int kRowsBlocks = 64;

// word e = k * words + w of the block, for this lane's e = first, first + stride, ...; rows past n end the walk
struct RowsWalk {
    uint32_t k, w, dk, dw;
    RM_D RowsWalk(uint32_t words)
    {
        const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
        k = first / words;
        w = first - k * words;
        dk = stride / words;
        dw = stride - dk * words;
    }
    RM_D void step(uint32_t words)
    {
        k += dk; // (k < n < 2^31 and dk < 2^14: no wrap)
        w += dw;
        if (w >= words) {
            w -= words;
            ++k;
        }
    }
};

// out word e is word e % words of row nodes[e / words]; a node outside 0 .. n_rows-1 gives 0.  With totals_out, the first lane
// copies the totals
__global__ void __launch_bounds__(256) k_rows_gather(const int64_t *__restrict__ table, int words, int n_rows, const int32_t *__restrict__ nodes, int n,
                                                     int64_t *__restrict__ out, const rm_stats_totals *__restrict__ totals,
                                                     rm_stats_totals *__restrict__ totals_out)
{
    const uint32_t W = uint32_t(words);
    for (RowsWalk at(W); at.k < uint32_t(n); at.step(W)) {
        const int32_t node = nodes[at.k];
        int64_t v = 0;
        if (node >= 0 && node < n_rows) v = table[size_t(node) * W + at.w];
        out[size_t(at.k) * W + at.w] = v;
    }
    if (totals_out && blockIdx.x == 0 && threadIdx.x == 0) *totals_out = *totals;
}

// the mirror image: src word e goes to word e % words of row nodes[e / words]; an entry whose node is outside the table is skipped.
// The host stages every entry with its node's FINAL record, so duplicates write equal values
__global__ void __launch_bounds__(256) k_rows_scatter(int64_t *__restrict__ table, int words, int n_rows, const int32_t *__restrict__ nodes, int n,
                                                      const int64_t *__restrict__ src)
{
    const uint32_t W = uint32_t(words);
    for (RowsWalk at(W); at.k < uint32_t(n); at.step(W)) {
        const int32_t node = nodes[at.k];
        if (node < 0 || node >= n_rows) continue;
        table[size_t(node) * W + at.w] = src[size_t(at.k) * W + at.w];
    }
}

static dim3 rows_grid(int words, int n)
{
    const size_t lanes = size_t(std::max(n, 0)) * size_t(words);
    return dim3(unsigned(std::max<size_t>(1, std::min<size_t>(kRowsBlocks, (lanes + 255u) / 256u))));
}

hipError_t launch_rows_gather(hipStream_t s, const int64_t *table, int words, int n_rows, const int32_t *nodes, int n, int64_t *out,
                              const rm_stats_totals *totals, rm_stats_totals *totals_out)
{
    if (words < 1 || (totals_out && !totals)) return hipErrorInvalidValue;
    if (n < 1 && !totals_out) return hipSuccess;
    RM_KLAUNCH(k_rows_gather, rows_grid(words, n), dim3(256), 0, s, table, words, n_rows, nodes, std::max(n, 0), out, totals, totals_out);
    return hipGetLastError();
}

hipError_t launch_rows_scatter(hipStream_t s, int64_t *table, int words, int n_rows, const int32_t *nodes, int n, const int64_t *src)
{
    if (words < 1) return hipErrorInvalidValue;
    if (n < 1) return hipSuccess;
    RM_KLAUNCH(k_rows_scatter, rows_grid(words, n), dim3(256), 0, s, table, words, n_rows, nodes, n, src);
    return hipGetLastError();
}

} // namespace rm
