// op_reduce.h -- the last step of a parameter gradient in the convolution units (stem_conv, gshead, conv3x3, conv1x1): the partial sums their weight-gradient
// kernels leave in scratch, [parts][M] with M = the weight's MW sums followed by the bias's, are added in index order, in groups of `group` and then the
// groups (DESIGN.md "Parameter-gradient reduction").  No atomics; every sum has a fixed order: the same bits on every run.  The group size is the
// including unit's own constant: it decides which adds are made, so it defines the bits.  The only arithmetic here is a plain add: the header is
// indifferent to the contraction setting of the unit that includes it.
#pragma once
#include "op_common.h"

namespace {

constexpr int SUM_THREADS = 256;  // of k_sum_partials alone: an op's own block size may change without this one following it

// scratch as sum_partials reads and writes it: the partials [parts][M], then (where parts > group) the group sums [ceil(parts / group)][M]
inline size_t partials_scratch_bytes(size_t parts, int group, size_t M) { return 4 * M * (parts + cdiv(parts, group)); }

// out[g][j] = sum over parts t in [g * group, min(parts, (g + 1) * group)) of in[t][j], in index order; g = blockIdx.x, one thread per j.  With
// dw != NULL (the last stage, one group) the M sums go to dw (j < MW) and db instead.
__global__ __launch_bounds__(SUM_THREADS) void k_sum_partials(const float *__restrict__ in, int parts, int group, int M, int MW, float *__restrict__ out,
                                                              float *__restrict__ dw, float *__restrict__ db) {
    const int j = threadIdx.x + (int)blockIdx.y * SUM_THREADS, g = (int)blockIdx.x;
    if (j >= M) return;
    const int t0 = g * group, t1 = min(parts, t0 + group);
    float s = 0.f;
#pragma unroll 8
    for (int t = t0; t < t1; t++) s += in[(size_t)t * M + j];  // (unrolled: the loads in flight together, the adds in index order)
    if (dw != nullptr) {
        if (j < MW) dw[j] = s; else db[j - MW] = s;
    } else {
        out[(size_t)g * M + j] = s;
    }
}

// dw[0..MW), db[0..M - MW) from partials [parts][M]: one launch where parts <= group, else the group sums (to partials + parts * M) and their sum.
// The second stage adds up to 2^31 / group sums in one thread per j: a few thousand for the shapes these ops are for (a full-resolution stereo batch).
// (`partials` is not const: the group sums are written behind them)
inline void sum_partials(float *partials, int parts, int group, int M, int MW, float *dw, float *db, hipStream_t s) {
    const dim3 block(SUM_THREADS);
    const unsigned jb = (unsigned)cdiv(M, SUM_THREADS);  // grid y: 129 for the largest M of these ops, conv1x1's 128 * (256 + 1)
    const float *in = partials;
    if (parts > group) {
        const int groups = (int)cdiv(parts, group);
        float *stage = partials + (size_t)parts * M;
        hipLaunchKernelGGL(k_sum_partials, dim3((unsigned)groups, jb), block, 0, s, in, parts, group, M, MW, stage, (float *)nullptr, (float *)nullptr);
        in = stage;
        parts = groups;
    }
    hipLaunchKernelGGL(k_sum_partials, dim3(1, jb), block, 0, s, in, parts, parts, M, MW, (float *)nullptr, dw, db);
}

}  // namespace
