// heads_kernels.hip -- GATConv attention of the edge-regret GNN for head counts other than 8 on MI355X (gfx950), hand-written
// HIP, fp32.  embed_dim stays 128, so H in {1, 2, 4, 16} heads have F = 128 / H in {128, 64, 32, 8} features each; every dense
// block of the model (embedding, fc, feed-forward, BatchNorms, decision layer, training GEMMs) keeps its shape and its kernel.
//
// Replaces (reference file:line, /root/reference/gnngls/...):
//   models.py:23      dgl.nn.GATConv(embed_dim, embed_dim // n_heads, n_heads) on the line graph of K_n, forward and backward
//   models.py:59-61   n_heads AttentionLayers (the reference's layer count is its head count)
//
// The 8-head kernels (model_kernels.hip gat_rows_kernel, train_kernels.hip gat_bwd_rows_kernel) keep softmax statistics per SLOT of
// 16 columns, and every consumer reads the statistics of column c from slot c / 16 (ffn_fused_kernel, ffn_fused_bf16x3_kernel,
// gat_combine_train_kernel, gat_bwd_combine_kernel, colsum CS_HEADSCALE).  The kernels here keep those consumers unchanged:
//   F >= 16 (H <= 8): a head covers F / 16 whole slots; its statistics are written into each of them (exact for every consumer).
//   F == 8  (H = 16): two heads share a slot.  The attention kernel writes per-head statistics [2][M][2 x 16] of its own;
//                     gat_heads_merge16_kernel merges the two sides per head and hands the consumers the finished GATConv output
//                     in side 0 with shift 0 / sum 1 and zeros with sum 0 in side 1, which their log-sum-exp merge returns unchanged:
//                     (x * 1 + 0 * 1) * (1 / (1 * 1 + 0 * 1)) = x, exactly (exp(0) = 1 exactly, no contraction: -ffp-contract=off).
//                     Training keeps its own merge (g, h1, per-head statistics) and its own backward combine / attention-vector sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heads_kernels.h"
#include "model_policy.h"

namespace gnngls {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float kSlope = 0.2f;                  // GATConv negative_slope default
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ int pair_rank(int i, int j, int n) {   // i < j, rank in itertools.combinations order
    return i * n - ((i * (i + 1)) >> 1) + (j - i - 1);
}

__device__ __forceinline__ float row16_sum(float v) {   // inclusive prefix over the 16-lane DPP row; lane 15 holds the total
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));   // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));   // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));   // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));   // row_shr:8
    return v;
}

int grid_cap(long want, int cap) {
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}
int ew_grid(long M) { return grid_cap((M * 32 + 255) / 256, 256 * 16); }
}  // namespace

// ---------------------------------------------------------------------------------------------
// Forward: one workgroup per (instance b, TSP row i, column group), as gat_rows_kernel.  The workgroup stages CW columns (whole
// heads) of the row's n - 1 source nodes {i,k} in LDS, computes el / er over each head's F features, the exact row maxima (top-2
// trick: excluding k = j) and the factorised weight tables, then aggregates on v_mfma_f32_16x16x4_f32: one unit = (16
// destinations, 64 columns = 4 MFMA column blocks).  For F >= 16 the column blocks of one head share the weights operand (the MFMA
// count per layer is that of the 8-head kernel); for F == 8 a 16-column block spans two heads and takes two MFMAs, each with the
// other head's 8 columns of the B operand zeroed (exact: the zeroed columns add w * 0 = 0).
// ---------------------------------------------------------------------------------------------
// HeadShape<F>, the carve of a workgroup: model_policy.h
template <int F>
__global__ __launch_bounds__(512) void gat_heads_rows_kernel(const float *__restrict__ ft, const float *__restrict__ attn_l,
                                                             const float *__restrict__ attn_r, int n, float *__restrict__ part,
                                                             float *__restrict__ part_ms, float *__restrict__ hms) {
    using S = HeadShape<F>;
    constexpr int CW = S::CW, HS = S::HS, HG = S::HG, LDF = S::LDF, UH = S::UH, UNITS = S::UNITS, LP = S::LP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = n * (n - 1) / 2, ns = n - 1;
    const int grp = blockIdx.x % HG;
    const int b = blockIdx.x / (n * HG), i = (blockIdx.x / HG) % n;
    const int c0 = grp * CW, hb = c0 / F;                    // first column / first head of the workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nthreads = blockDim.x, nwaves = nthreads >> 6;
    float *ftS = reinterpret_cast<float *>(smem);            // [ns][LDF]
    float *elS = ftS + (size_t)ns * LDF;                     // [ns][HS]
    float *erS = elS + (size_t)ns * HS;                      // [ns][HS]
    float *eaS = erS + (size_t)ns * HS;                      // [ns][HS] exp(el - max1)
    float *ebS = eaS + (size_t)ns * HS;                      // [ns][HS] exp(0.2 (el - max1))
    float *top = ebS + (size_t)ns * HS;                      // [HS][4]: max1, max2, argmax1 (int bits), direct-path flag
    int *nodeS = reinterpret_cast<int *>(top + HS * 4);      // [ns] global node id of slot

    const float *ftb = ft + (size_t)b * N * kD;
    for (int s = tid; s < ns; s += nthreads) {
        const int k = s < i ? s : s + 1;
        nodeS[s] = k < i ? pair_rank(k, i, n) : pair_rank(i, k, n);
    }
    __syncthreads();
    constexpr int SB = 8, V4 = CW / 4;
    for (int q0 = tid; q0 < ns * V4; q0 += nthreads * SB) {
        f32x4 v[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int q = q0 + u * nthreads;
            if (q < ns * V4) v[u] = *reinterpret_cast<const f32x4 *>(ftb + (size_t)nodeS[q / V4] * kD + c0 + (q % V4) * 4);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int q = q0 + u * nthreads;
            if (q < ns * V4) *reinterpret_cast<f32x4 *>(ftS + (size_t)(q / V4) * LDF + (q % V4) * 4) = v[u];
        }
    }
    __syncthreads();
    {   // el / er = <ft, attn_l / attn_r> over the head's F features: LP lanes per (source, head), reduced by shuffles (the loop
        // stride is a multiple of LP, so a lane group is always active together)
        constexpr int FL = F / LP;
        for (int q = tid; q < ns * HS * LP; q += nthreads) {
            const int item = q / LP, pl = q % LP;
            const int s = item / HS, h = item % HS;
            const float *f = ftS + (size_t)s * LDF + h * F + pl * FL;
            const float *al = attn_l + (hb + h) * F + pl * FL, *ar = attn_r + (hb + h) * F + pl * FL;
            float l = 0.f, r = 0.f;
#pragma unroll
            for (int v = 0; v < FL; v += 4) {
                const f32x4 fv = *reinterpret_cast<const f32x4 *>(f + v);
                const f32x4 a = *reinterpret_cast<const f32x4 *>(al + v), c = *reinterpret_cast<const f32x4 *>(ar + v);
#pragma unroll
                for (int u = 0; u < 4; ++u) { l = fmaf(fv[u], a[u], l); r = fmaf(fv[u], c[u], r); }
            }
#pragma unroll
            for (int o = 1; o < LP; o <<= 1) { l += __shfl_xor(l, o, 64); r += __shfl_xor(r, o, 64); }
            if (pl == 0) { elS[item] = l; erS[item] = r; }
        }
    }
    __syncthreads();
    if (tid < 32 * HS) {   // top-2 of el per head over the row's sources (gat_rows_kernel's merge of (max1, arg1, max2) triples)
        const int h = tid >> 5, l32 = tid & 31;
        float m1 = -INFINITY, m2 = -INFINITY; int a1 = -1;
        for (int s = l32; s < ns; s += 32) {
            const float v = elS[s * HS + h];
            if (v > m1) { m2 = m1; m1 = v; a1 = s; } else if (v > m2) { m2 = v; }
        }
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            const float om1 = __shfl_xor(m1, o, 32), om2 = __shfl_xor(m2, o, 32);
            const int oa1 = __shfl_xor(a1, o, 32);
            const bool take = om1 > m1 || (om1 == m1 && oa1 >= 0 && (a1 < 0 || oa1 < a1));
            const float lo1 = take ? m1 : om1;
            const float hi2 = take ? om2 : m2;
            if (take) { m1 = om1; a1 = oa1; }
            m2 = lo1 > hi2 ? lo1 : hi2;
        }
        if (l32 == 0) { top[h * 4 + 0] = m1; top[h * 4 + 1] = m2; top[h * 4 + 2] = __int_as_float(a1);
                        top[h * 4 + 3] = (m1 - m2 > 60.f) ? 1.f : 0.f; }
    }
    __syncthreads();
    for (int q = tid; q < ns * HS; q += nthreads) {
        const float d = (elS[q] - top[(q % HS) * 4]) * kLog2e;
        eaS[q] = __builtin_amdgcn_exp2f(d);
        ebS[q] = __builtin_amdgcn_exp2f(kSlope * d);
    }
    __syncthreads();

    const int n_dt = (ns + 15) >> 4;
    const int jl = lane & 15, kq = lane >> 4;
    float *pb = part + (size_t)b * N * kD;
    const size_t side_stride = (size_t)gridDim.x / (n * HG) * N;      // B*N nodes per side
    for (int unit = wave; unit < n_dt * UNITS; unit += nwaves) {
        const int dt = unit / UNITS, u0 = (unit % UNITS) * 64;           // u0: first column of the unit inside the workgroup's CW
        const int hu0 = u0 / F;                                          // first head of the unit inside the workgroup
        const int js = dt * 16 + jl;
        const int jsc = js < ns ? js : ns - 1;
        float er[UH], mm[UH], nm[UH], ws[UH], cpos[UH], cneg[UH];
        f32x4 acc[4];
        bool direct = false;
#pragma unroll
        for (int u = 0; u < UH; ++u) {
            const int h = hu0 + u;
            er[u] = erS[jsc * HS + h];
            const float m = ((__float_as_int(top[h * 4 + 2]) == js) ? top[h * 4 + 1] : top[h * 4 + 0]) + er[u];
            mm[u] = m > 0.f ? m : kSlope * m;                // LeakyReLU is monotone: max score = score of max el
            nm[u] = -mm[u] * kLog2e;
            ws[u] = 0.f;
            // exp(LeakyReLU(el + er) - mm) = max(exp(el - M) exp(er + M - mm), exp(0.2 (el - M)) exp(0.2 (er + M) - mm))
            const float t = er[u] + top[h * 4 + 0];
            cpos[u] = __builtin_amdgcn_exp2f(fminf(t - mm[u], 80.f) * kLog2e);
            cneg[u] = __builtin_amdgcn_exp2f(fminf(kSlope * t - mm[u], 80.f) * kLog2e);
            direct = direct || top[h * 4 + 3] != 0.f;        // wave-uniform
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < ns; s0 += 8) {                 // two groups of 4 sources per iteration
            float w[2][UH], bv[2][4];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int s = s0 + 4 * g + kq;
                const int sc = s < ns ? s : ns - 1;
                const bool live = (s < ns) && (s != js);     // no self loop, no padding
#pragma unroll
                for (int u = 0; u < UH; ++u) {
                    const int h = hu0 + u;
                    float x;
                    if (!direct) {
                        x = fmaxf(eaS[sc * HS + h] * cpos[u], ebS[sc * HS + h] * cneg[u]);
                    } else {
                        float v = elS[sc * HS + h] + er[u];
                        v = fmaxf(v, kSlope * v);            // LeakyReLU(x) = max(x, 0.2x)
                        x = __builtin_amdgcn_exp2f(fmaf(v, kLog2e, nm[u]));
                    }
                    x = live ? x : 0.f;
                    ws[u] += x;
                    w[g][u] = x;
                }
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) bv[g][cb] = ftS[(size_t)sc * LDF + u0 + 16 * cb + jl];
            }
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    if constexpr (F >= 16) {
                        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[g][(16 * cb) / F], bv[g][cb], acc[cb], 0, 0, 0);
                    } else {                                 // F = 8: columns 0-7 of the block are head 2 cb, 8-15 head 2 cb + 1
                        const float lo = jl < 8 ? bv[g][cb] : 0.f, hi = jl < 8 ? 0.f : bv[g][cb];
                        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[g][2 * cb], lo, acc[cb], 0, 0, 0);
                        acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[g][2 * cb + 1], hi, acc[cb], 0, 0, 0);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < UH; ++u) { ws[u] += __shfl_xor(ws[u], 16, 64); ws[u] += __shfl_xor(ws[u], 32, 64); }
        // C/D layout 16x16: col = lane&15 (feature), row = (lane>>4)*4 + reg (destination in the tile)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jd = dt * 16 + kq * 4 + r;
            if (jd < ns) {
                const int j = jd < i ? jd : jd + 1;
                float *po = pb + (i < j ? 0 : side_stride * kD) + (size_t)nodeS[jd] * kD + c0 + u0;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) po[16 * cb + jl] = acc[cb][r];
            }
        }
        if (kq == 0 && js < ns) {
            const int j = js < i ? js : js + 1;
            const size_t row = (i < j ? 0 : side_stride) + (size_t)b * N + nodeS[js];
            if constexpr (F >= 16) {                         // the head's statistics into every slot of its columns
                float *mo = part_ms + row * 16;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const int slot = (c0 + u0) / 16 + cb, u = (16 * cb) / F;
                    mo[slot] = mm[u]; mo[8 + slot] = ws[u];
                }
            } else {                                         // per-head statistics [2][M][16 + 16] for gat_heads_merge16_kernel
                float *mo = hms + row * 32;
#pragma unroll
                for (int u = 0; u < UH; ++u) { mo[hb + hu0 + u] = mm[u]; mo[16 + hb + hu0 + u] = ws[u]; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16 heads: the log-sum-exp merge of the two row partials per head, with gat_combine_train_kernel's arithmetic.
//   TRAIN = false: part side 0 <- GATConv output, side 1 <- 0, part_ms side 0 <- (0, 1), side 1 <- (0, 0) per slot, for the
//                  feed-forward launch's own merge (which then returns the output unchanged, see the head of this file)
//   TRAIN = true:  g = GATConv(h), h1 = h + g, att[m] = (row max, 1/Z) per head [M][16 + 16]
// ---------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ void gat_heads_merge16_kernel(float *part, const float *__restrict__ hms, float *__restrict__ part_ms,
                                         const float *__restrict__ h, long M, float *__restrict__ g, float *__restrict__ h1,
                                         float *__restrict__ att) {
    const long total = M * (kD / 4);
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long m = q >> 5;
        const int c4 = (int)(q & 31), hd = c4 >> 1;
        const float *ms0 = hms + m * 32, *ms1 = hms + (M + m) * 32;
        const float m0 = ms0[hd], s0 = ms0[16 + hd], m1 = ms1[hd], s1 = ms1[16 + hd];
        const float mx = m0 > m1 ? m0 : m1;
        const float a0 = __expf(m0 - mx), a1 = __expf(m1 - mx);
        const float inv = 1.f / (s0 * a0 + s1 * a1);
        const f32x4 p0 = *reinterpret_cast<const f32x4 *>(part + q * 4);
        const f32x4 p1 = *reinterpret_cast<const f32x4 *>(part + (M * kD) + q * 4);
        f32x4 gv;
#pragma unroll
        for (int v = 0; v < 4; ++v) gv[v] = (p0[v] * a0 + p1[v] * a1) * inv;
        if constexpr (TRAIN) {
            const f32x4 hv = *reinterpret_cast<const f32x4 *>(h + q * 4);
            f32x4 o;
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = hv[v] + gv[v];
            *reinterpret_cast<f32x4 *>(g + q * 4) = gv;
            *reinterpret_cast<f32x4 *>(h1 + q * 4) = o;
            if ((c4 & 1) == 0) { att[m * 32 + hd] = mx; att[m * 32 + 16 + hd] = inv; }
        } else {
            *reinterpret_cast<f32x4 *>(part + q * 4) = gv;
            *reinterpret_cast<f32x4 *>(part + (M * kD) + q * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c4 < 4) {                                    // 16 statistics per side and node: 4 per thread of the first four
                const float s = c4 >= 2 ? 1.f : 0.f;
                *reinterpret_cast<f32x4 *>(part_ms + m * 16 + c4 * 4) = f32x4{s, s, s, s};
                *reinterpret_cast<f32x4 *>(part_ms + (M + m) * 16 + c4 * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Backward: GATConv backward over the line graph of K_n (gat_bwd_rows_kernel's formulation), one workgroup per (instance b,
// TSP row u, head group), per head h of the row's nodes (destinations i and sources j at once):
//     a_ij = exp(LeakyReLU(el_j + er_i) - max_i) / Z_i,  t_ij = <dOut_i, ft_j>_h,  c_i = <dOut_i, out_i>_h
//     ds_ij = a_ij (t_ij - c_i) LeakyReLU'(el_j + er_i);  P_j = sum_i a_ij dOut_i,  del_j = sum_i ds_ij,  der_i = sum_j ds_ij
// The dOut columns of the head group are staged in LDS; ft comes from memory once per source tile.  WS wavefronts share a head
// (F >= 32: 4 waves per workgroup): wave w takes the source tiles st = w mod WS, w + WS, ...; for each, it walks all destination
// tiles with T = dOut * ft^T on the MFMA (F / 4 steps) and feeds the attention weights back into a^T * dOut (F / 16 column blocks,
// one for F = 8 with the neighbour head's columns zeroed).  P / del of a source tile leave the registers when the tile is done;
// der accumulates per wave in LDS and the WS partials are summed in fixed order at the end (deterministic).
// Outputs: P [2][M][128] by side; d el / d er into `dlr` in the layout of the consumers: F >= 16 the slot layout [2][M][8 + 8]
// of gat_bwd_combine_kernel (replicated over the head's slots), F = 8 per head [2][M][16 + 16] (gat_heads_bwd_combine16_kernel).
// ---------------------------------------------------------------------------------------------
// The workgroup shape BwdShape<F> and the LDS carve below (heads_bwd_lds<F>) are model_policy.h's, shared with the plan.
static_assert(BwdShape<128>::WAVES * 64 <= 512 && BwdShape<64>::WAVES * 64 <= 512 && BwdShape<32>::WAVES * 64 <= 512 &&
              BwdShape<8>::WAVES * 64 <= 512, "gat_heads_bwd_rows_kernel's launch bound");
static_assert(BwdShape<128>::LDG % 4 == 0 && BwdShape<64>::LDG % 4 == 0, "16-byte LDS rows");

template <int F>
__global__ __launch_bounds__(512) void gat_heads_bwd_rows_kernel(const float *__restrict__ ft, const float *__restrict__ dout,
                                                                 const float *__restrict__ gout, const float *__restrict__ att,
                                                                 const float *__restrict__ attn_l, const float *__restrict__ attn_r,
                                                                 int n, float *__restrict__ P, float *__restrict__ dlr) {
    using S = BwdShape<F>;
    constexpr int CW = S::CW, HB = S::HB, WS = S::WS, LDG = S::LDG, KB = S::KB, LP = S::LP, ATS = S::ATS;
    constexpr int groups = kD / CW, nthreads = 64 * S::WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int N = n * (n - 1) / 2;
    const int ns = n - 1, nt = (ns + 15) >> 4;
    const int grp = blockIdx.x % groups, bu = blockIdx.x / groups;
    const int b = bu / n, u = bu % n;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = grp * CW;
    f32x4 *stS = reinterpret_cast<f32x4 *>(smem);                 // [ns][HB] (er, -max*log2e, 1/Z, c)
    float *dgS = reinterpret_cast<float *>(stS + (size_t)ns * HB); // [ns][LDG] columns c0 .. c0+CW of dOut
    float *elS = dgS + (size_t)ns * LDG;                          // [ns][HB]
    float *derS = elS + (size_t)ns * HB;                          // [WAVES][ns] per-wave partial d er
    int *nodeS = reinterpret_cast<int *>(derS + (size_t)S::WAVES * ns);   // [ns] line-graph node of slot s
    const size_t Mtot = (size_t)gridDim.x / (n * groups) * N;     // B*N rows per side
    const size_t base = (size_t)b * N;

    for (int s = tid; s < ns; s += nthreads) {
        const int k = s < u ? s : s + 1;
        nodeS[s] = k < u ? pair_rank(k, u, n) : pair_rank(u, k, n);
    }
    for (int q = tid; q < S::WAVES * ns; q += nthreads) derS[q] = 0.f;
    __syncthreads();
    constexpr int SB = 4, V4 = CW / 4;
    for (int q0 = tid; q0 < ns * V4; q0 += nthreads * SB) {
        f32x4 vd[SB];
#pragma unroll
        for (int k = 0; k < SB; ++k) {
            const int q = q0 + k * nthreads;
            if (q < ns * V4) vd[k] = *reinterpret_cast<const f32x4 *>(dout + (base + nodeS[q / V4]) * kD + c0 + (q % V4) * 4);
        }
#pragma unroll
        for (int k = 0; k < SB; ++k) {
            const int q = q0 + k * nthreads;
            if (q < ns * V4) *reinterpret_cast<f32x4 *>(dgS + (size_t)(q / V4) * LDG + (q % V4) * 4) = vd[k];
        }
    }
    __syncthreads();
    {   // el, er and c = <dOut, out> per (slot, head): LP lanes per pair, 16 (F = 8: 8) features each, reduced by shuffles
        constexpr int FL = F / LP;
        for (int q = tid; q < ns * HB * LP; q += nthreads) {
            const int item = q / LP, pl = q % LP;
            const int s = item / HB, hl = item % HB, hh = c0 / F + hl;
            const int col = hh * F + pl * FL;
            const size_t row = (base + nodeS[s]) * kD;
            const float *d = dgS + (size_t)s * LDG + hl * F + pl * FL;
            float l = 0.f, r = 0.f, c = 0.f;
#pragma unroll
            for (int v = 0; v < FL; v += 4) {
                const f32x4 fv = *reinterpret_cast<const f32x4 *>(ft + row + col + v);
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(gout + row + col + v);
                const f32x4 dv = *reinterpret_cast<const f32x4 *>(d + v);
                const f32x4 al = *reinterpret_cast<const f32x4 *>(attn_l + col + v), ar = *reinterpret_cast<const f32x4 *>(attn_r + col + v);
#pragma unroll
                for (int k = 0; k < 4; ++k) { l = fmaf(fv[k], al[k], l); r = fmaf(fv[k], ar[k], r); c = fmaf(dv[k], gv[k], c); }
            }
#pragma unroll
            for (int o = 1; o < LP; o <<= 1) { l += __shfl_xor(l, o, 64); r += __shfl_xor(r, o, 64); c += __shfl_xor(c, o, 64); }
            if (pl == 0) {
                const float *a = att + (base + nodeS[s]) * ATS;
                const int am = F >= 16 ? hh * (F / 16) : hh;            // the head's (first) statistics column
                elS[item] = l;
                stS[item] = f32x4{r, -a[am] * kLog2e, a[ATS / 2 + am], c};
            }
        }
    }
    __syncthreads();

    const int jl = lane & 15, q4 = lane >> 4;
    const int hl = w / WS, hh = c0 / F + hl;                      // this wave's head (in the group / global)
    const int cl = hl * F, cg = hh * F;                           // its first column in the LDS tile / in the row
    auto out_row = [&](int s) -> size_t { return ((u <= s) ? 0 : Mtot) + base + nodeS[s]; };
    // F = 8: lanes q4 >= 2 supply zero features of T, lanes jl >= 8 zero columns of P (the other head of the 16-column block)
    const bool tlive = F >= 16 || q4 < 2, plive = F >= 16 || jl < 8;
    for (int st = w % WS; st < nt; st += WS) {
        const int j = st * 16 + jl, jc = j < ns ? j : ns - 1;
        const float el_j = elS[jc * HB + hl];
        const float *ftj = ft + (base + nodeS[jc]) * kD + cg;
        f32x4 bft[KB], accP[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            bft[kb] = tlive ? *reinterpret_cast<const f32x4 *>(ftj + 16 * kb + 4 * q4) : f32x4{0.f, 0.f, 0.f, 0.f};
            accP[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float del = 0.f;
        for (int dt = 0; dt < nt; ++dt) {
            const int ia = dt * 16 + jl, iac = ia < ns ? ia : ns - 1;
            f32x4 T = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                const f32x4 adg = tlive ? *reinterpret_cast<const f32x4 *>(dgS + (size_t)iac * LDG + cl + 16 * kb + 4 * q4)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) T = __builtin_amdgcn_mfma_f32_16x16x4f32(adg[ks], bft[kb][ks], T, 0, 0, 0);
            }
            // T[r] = t_ij for destination i = 16*dt + 4*q4 + r, source j = 16*st + jl
            float av[4];
            int icl[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = dt * 16 + 4 * q4 + r, ic = i < ns ? i : ns - 1;
                icl[r] = ic;
                const f32x4 sv = stS[ic * HB + hl];
                const float x = el_j + sv[0];
                const float lx = fmaxf(x, kSlope * x);
                float a = __builtin_amdgcn_exp2f(fmaf(lx, kLog2e, sv[1])) * sv[2];
                const bool live = (i < ns) && (j < ns) && (i != j);
                a = live ? a : 0.f;
                const float ds = a * (T[r] - sv[3]) * (x > 0.f ? 1.f : kSlope);
                av[r] = a;
                del += ds;
                const float rs = row16_sum(ds);                          // d er_i: sum over the 16 source lanes
                if (jl == 15 && i < ns) derS[w * ns + i] += rs;
            }
            // P[j][:] += sum_i a_ij dOut_i[:]: the T accumulator layout is the A-operand layout of step r of a^T * dOut
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float bdg = plive ? dgS[(size_t)icl[r] * LDG + cl + 16 * kb + jl] : 0.f;
                    accP[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bdg, accP[kb], 0, 0, 0);
                }
        }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        if (q4 == 0 && j < ns) {
            float *o = dlr + out_row(j) * ATS;
            if constexpr (F >= 16) {
#pragma unroll
                for (int k = 0; k < F / 16; ++k) o[hh * (F / 16) + k] = del;
            } else {
                o[hh] = del;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jr = st * 16 + 4 * q4 + r;
            if (jr < ns && plive) {
                float *po = P + out_row(jr) * kD + cg + jl;
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) po[16 * kb] = accP[kb][r];
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < ns * HB; q += nthreads) {                // d er: the WS wave partials of a head in fixed order
        const int s = q / HB, h2 = q % HB, hg = c0 / F + h2;
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < WS; ++k) d += derS[(h2 * WS + k) * ns + s];
        float *o = dlr + out_row(s) * ATS + ATS / 2;
        if constexpr (F >= 16) {
#pragma unroll
            for (int k = 0; k < F / 16; ++k) o[hg * (F / 16) + k] = d;
        } else {
            o[hg] = d;
        }
    }
}

// 16 heads: dft = P0 + P1 + (del0 + del1) * attn_l + (der0 + der1) * attn_r per head (gat_bwd_combine_kernel's arithmetic);
// dl / dr [M][16] = the summed d el / d er per head
__global__ void gat_heads_bwd_combine16_kernel(const float *__restrict__ P, const float *__restrict__ dlr,
                                               const float *__restrict__ attn_l, const float *__restrict__ attn_r, long M,
                                               float *__restrict__ dft, float *__restrict__ dl, float *__restrict__ dr) {
    const long total = M * (kD / 4);
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
        const long m = q >> 5;
        const int c4 = (int)(q & 31), hd = c4 >> 1, c = c4 * 4;
        const float *d0 = dlr + m * 32, *d1 = dlr + (M + m) * 32;
        const float l = d0[hd] + d1[hd], r = d0[16 + hd] + d1[16 + hd];
        const f32x4 p0 = *reinterpret_cast<const f32x4 *>(P + q * 4);
        const f32x4 p1 = *reinterpret_cast<const f32x4 *>(P + M * kD + q * 4);
        f32x4 o;
#pragma unroll
        for (int v = 0; v < 4; ++v) o[v] = (p0[v] + p1[v]) + l * attn_l[c + v] + r * attn_r[c + v];
        *reinterpret_cast<f32x4 *>(dft + q * 4) = o;
        if ((c4 & 1) == 0) { dl[m * 16 + hd] = l; dr[m * 16 + hd] = r; }
    }
}

// 16 heads: the attn_l / attn_r gradient sums, partial[block][k][c] = sum over the block's rows of X[m,c] * Y_k[m, c/8] in fp64
// (colsum_kernel's CS_HEADSCALE with 8-column heads; the same partial layout, finished by launch_colsum_store)
__global__ __launch_bounds__(256) void colsum_heads16_kernel(const float *__restrict__ X, const float *__restrict__ Y,
                                                             const float *__restrict__ Y2, long M, double *__restrict__ partial) {
    __shared__ double red[2 * 1024];
    constexpr int C = kD, cg = C / 4, rl = 256 / cg;
    const int tid = threadIdx.x;
    const int c = (tid % cg) * 4, r = tid / cg;
    double a0[4] = {0, 0, 0, 0}, a1[4] = {0, 0, 0, 0};
    for (long m = (long)blockIdx.x * rl + r; m < M; m += (long)gridDim.x * rl) {
        const f32x4 x = *reinterpret_cast<const f32x4 *>(X + m * C + c);
        const double s = (double)Y[m * 16 + (c >> 3)], s2 = (double)Y2[m * 16 + (c >> 3)];
#pragma unroll
        for (int v = 0; v < 4; ++v) { a0[v] += (double)x[v] * s; a1[v] += (double)x[v] * s2; }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) { red[r * C + c + v] = a0[v]; red[1024 + r * C + c + v] = a1[v]; }
    __syncthreads();
    for (int q = tid; q < 2 * C; q += 256) {
        const int k = q / C, cc = q % C;
        double s = 0.0;
        for (int rr = 0; rr < rl; ++rr) s += red[k * 1024 + rr * C + cc];
        partial[((long)blockIdx.x * 2 + k) * C + cc] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static_assert(HeadShape<128>::UNITS == 2 && HeadShape<64>::UNITS == 1 && HeadShape<32>::UNITS == 1 && HeadShape<8>::UNITS == 1,
              "gat_heads_rows_units() counts the 64-column units of a workgroup");

template <int F>
static hipError_t launch_rows(const float *ft, const float *attn_l, const float *attn_r, int B, int n, int waves, float *part,
                              float *part_ms, float *hms, hipStream_t st) {
    using S = HeadShape<F>;
    const size_t lds = heads_rows_lds<F>(n);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gat_heads_rows_kernel<F>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gat_heads_rows_kernel<F>, dim3((unsigned)(B * n * S::HG)), dim3(64 * waves), lds, st, ft, attn_l, attn_r, n,
                       part, part_ms, hms);
    return hipGetLastError();
}

hipError_t launch_gat_heads_rows(const float *ft, const float *attn_l, const float *attn_r, int B, int n, int n_heads, int waves,
                                 float *part, float *part_ms, float *hms, hipStream_t st) {
    if (n < 3 || n > kMaxNodes || waves < 4 || waves > 8) return hipErrorInvalidValue;
    switch (n_heads) {
    case 1: return launch_rows<128>(ft, attn_l, attn_r, B, n, waves, part, part_ms, hms, st);
    case 2: return launch_rows<64>(ft, attn_l, attn_r, B, n, waves, part, part_ms, hms, st);
    case 4: return launch_rows<32>(ft, attn_l, attn_r, B, n, waves, part, part_ms, hms, st);
    case 16: return launch_rows<8>(ft, attn_l, attn_r, B, n, waves, part, part_ms, hms, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_gat_heads_merge16(float *part, const float *hms, float *part_ms, long M, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(gat_heads_merge16_kernel<false>, dim3(ew_grid(M)), dim3(256), 0, st, part, hms, part_ms, nullptr, M, nullptr,
                       nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_gat_heads_merge16_train(const float *part, const float *hms, const float *h, long M, float *g, float *h1, float *att,
                                          hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(gat_heads_merge16_kernel<true>, dim3(ew_grid(M)), dim3(256), 0, st, const_cast<float *>(part), hms, nullptr,
                       h, M, g, h1, att);
    return hipGetLastError();
}

template <int F>
static hipError_t launch_bwd(const float *ft, const float *dout, const float *gout, const float *att, const float *attn_l,
                             const float *attn_r, int B, int n, size_t lds, float *P, float *dlr, hipStream_t st) {
    using S = BwdShape<F>;
    if (lds != heads_bwd_lds<F>(n)) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(gat_heads_bwd_rows_kernel<F>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gat_heads_bwd_rows_kernel<F>, dim3((unsigned)(B * n * (kD / S::CW))), dim3(64 * S::WAVES), lds, st, ft, dout,
                       gout, att, attn_l, attn_r, n, P, dlr);
    return hipGetLastError();
}

hipError_t launch_gat_heads_bwd_rows(const float *ft, const float *dout, const float *gout, const float *att, const float *attn_l,
                                     const float *attn_r, int B, int n, int n_heads, size_t lds, float *P, float *dlr, hipStream_t st) {
    if (n < 3 || n > kMaxNodes) return hipErrorInvalidValue;
    switch (n_heads) {
    case 1: return launch_bwd<128>(ft, dout, gout, att, attn_l, attn_r, B, n, lds, P, dlr, st);
    case 2: return launch_bwd<64>(ft, dout, gout, att, attn_l, attn_r, B, n, lds, P, dlr, st);
    case 4: return launch_bwd<32>(ft, dout, gout, att, attn_l, attn_r, B, n, lds, P, dlr, st);
    case 16: return launch_bwd<8>(ft, dout, gout, att, attn_l, attn_r, B, n, lds, P, dlr, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_gat_heads_bwd_combine16(const float *P, const float *dlr, const float *attn_l, const float *attn_r, long M,
                                          float *dft, float *dl, float *dr, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(gat_heads_bwd_combine16_kernel, dim3(ew_grid(M)), dim3(256), 0, st, P, dlr, attn_l, attn_r, M, dft, dl, dr);
    return hipGetLastError();
}

hipError_t launch_colsum_heads16(const float *X, const float *Y, const float *Y2, long M, double *partial, int nblocks,
                                 hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(colsum_heads16_kernel, dim3(nblocks), dim3(256), 0, st, X, Y, Y2, M, partial);
    return hipGetLastError();
}

}  // namespace gnngls
