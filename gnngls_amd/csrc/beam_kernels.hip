// beam_kernels.hip -- beam-search decoding of tours from any edge score on MI355X (gfx950), hand-written HIP.
//
// The reference has no counterpart (its paper compares against the greedy / beam-search decoders of the edge-heatmap models).
// include/gnngls_hip.h states the definition (gnngls_beam_search), gnngls_amd.host.beam_search restates it in NumPy and the device
// matches it bit for bit.
//
// One workgroup of min(width, 16) wavefronts per instance runs all n - 1 steps, the close and the selection of a launch.  The
// beams' scores, last nodes and (where they fit, beam_masks_in_lds) visited bitmasks live in LDS, double-buffered.  A step never
// stores its up to width * n candidate keys: every pass over the candidates re-forms them -- wavefront k % 16 takes beam k, lane l
// node l + 64 s, one coalesced read of row last_k of S and one broadcast bitmask word per 64 nodes, eight such pieces in flight.
//
//   SELECT.  A key is the fp64 sum mapped to a uint64 of the same order (a zero first taken as +0.0, so that -0.0 and +0.0 tie).
//            The candidate of rank `width` in (key, k, j) is found by a radix select over the digit string 11+11+11+11+11+9 bits
//            of the key, then 10 bits of k, then 10 bits of j: per digit an LDS histogram of the candidates that match the digits
//            found so far (one atomic per wavefront where its lanes agree on the bin, as they do on sign and exponent), and a
//            scan of the 2,048 bins by wavefront 0.  The passes end as soon as the bins up to the chosen one hold exactly the
//            wanted count -- with distinct keys at the latest after the key's last digit; only ties across the cut read k and j.
//   EMIT.    One more pass appends every candidate at or below the cut to an LDS buffer (one atomic per wavefront and 64 nodes).
//   SORT.    Those at most 1,024 (key, id) pairs are ranked by counting, every thread one pair against all (broadcast reads);
//            the rank is the new beam's index.  c, last, the back-pointer (parent rank, node) -> global workspace; the bitmasks
//            of the new beams are then copied from their parents by all threads.
//   CLOSE.   One thread per final beam walks the back-pointers once, writes the tour, adds S[last, depot] and, given D, sums the
//            tour's cost left to right as gnngls_tour_cost does; wavefront 0 picks the best in (score | cost, rank).
//
// Global memory this workgroup writes and re-reads (back-pointers, tours, spilled bitmasks) is its own: plain stores, then the
// workgroup's barrier, as aco_kernel treats tau.
//
// [exact] the only fp64 operations are single adds (contraction off).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "beam_kernels.h"

#pragma clang fp contract(off)

namespace gnngls {

namespace {

constexpr int kLanes = 64;
constexpr int kBins = 2048;              // 11-bit digits; wavefront 0 scans 32 bins per lane
constexpr int kUnroll = 8;                // (beam, word) pairs whose loads are in flight together
constexpr int kIdBits = 10;              // id = k << 10 | j
constexpr uint32_t kIdAll = 0xFFFFFFFFu;

struct BeamCtl {
    uint32_t bin, need, fin, count;      // the radix pass's answer; the emit counter
    int32_t bad, best;
};

__host__ __device__ inline size_t beam_r16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline int beam_words(int n) { return (n + kLanes - 1) / kLanes; }
__host__ __device__ inline size_t beam_fixed_lds(int W) {
    return beam_r16(sizeof(BeamCtl)) + (size_t)kBins * sizeof(uint32_t) + 3 * beam_r16((size_t)W * 8) + 3 * beam_r16((size_t)W * 4);
}
__host__ __device__ inline size_t beam_mask_bytes(int n, int W) { return beam_r16((size_t)2 * W * beam_words(n) * sizeof(uint64_t)); }
__host__ __device__ inline size_t beam_bp_bytes(int n, int W) { return beam_r16((size_t)(n - 1) * W * sizeof(uint32_t)); }
__host__ __device__ inline size_t beam_tours_bytes(int n, int W) { return beam_r16((size_t)W * (n + 1) * sizeof(int32_t)); }

// the sum as a uint64 whose unsigned order is the fp64 order of the sums (no NaN arises from finite S); zeros -> +0.0
__device__ __forceinline__ uint64_t key_of(double c, double s) {
    const double v = c + s;
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if ((b << 1) == 0ull) b = 0ull;
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

__device__ __forceinline__ double value_of(uint64_t k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull)));
}

// f(valid, key, k, j) for every (beam k of this wavefront, node j of this lane), all lanes together (f may ballot)
template <class F>
__device__ __forceinline__ void for_candidates(const double *S, int n, int nw, int nb, const double *c, const int32_t *last,
                                               const uint64_t *mask, int wave, int nwaves, int lane, F f) {
    // The (beam, word) pairs of this wavefront, kUnroll at a time: all their loads are issued before the first key is formed, so one
    // L2 round trip serves kUnroll row pieces.  The loads are unconditional (a select around a load would serialise them): a lane
    // beyond n reads column n - 1 and a visited node reads its entry, the diagonal among them, but no such value is ever used.
    const int mine = nb > wave ? (nb - wave + nwaves - 1) / nwaves : 0;
    const int items = mine * nw;
    int k = wave, s = 0;
    for (int i0 = 0; i0 < items; i0 += kUnroll) {
        double sv[kUnroll], ck[kUnroll];
        uint64_t mw[kUnroll];
        int kk[kUnroll], jj[kUnroll];
        bool in[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            in[u] = i0 + u < items;
            kk[u] = in[u] ? k : wave;
            const int su = in[u] ? s : 0;
            jj[u] = lane + kLanes * su;
            mw[u] = mask[(size_t)kk[u] * nw + su];
            ck[u] = c[kk[u]];
            sv[u] = S[(size_t)last[kk[u]] * n + (jj[u] < n ? jj[u] : n - 1)];
            if (++s == nw) { s = 0; k += nwaves; }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const bool valid = in[u] && jj[u] < n && !((mw[u] >> lane) & 1ull);
            f(valid, valid ? key_of(ck[u], sv[u]) : 0ull, kk[u], jj[u]);
        }
    }
}

__device__ __forceinline__ void hist_add(uint32_t *hist, bool m, uint32_t digit, int lane) {
    const unsigned long long bm = __ballot(m);
    if (bm == 0ull) return;
    const int first = __ffsll((long long)bm) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)digit, first);
    if (__ballot(m && digit != d0) == 0ull) {
        if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll((long long)bm));
    } else if (m) {
        atomicAdd(&hist[digit], 1u);
    }
}

// wavefront 0: the bin in which the running count reaches `need`; -> ctl->bin, ctl->need (the rank inside the bin), ctl->fin
__device__ __forceinline__ void find_bin(const uint32_t *hist, uint32_t need, int lane, BeamCtl *ctl) {
    constexpr int per = kBins / kLanes;
    uint32_t s = 0;
    for (int q = 0; q < per; ++q) s += hist[lane * per + ((q + lane) & (per - 1))];     // rotated: one bank per lane
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += t;
    }
    const unsigned long long over = __ballot(incl >= need);
    if (over == 0ull) {                                   // never: need <= the number of matching candidates
        if (lane == 0) { ctl->bin = 0; ctl->need = 0; ctl->fin = 1; }
        return;
    }
    if (lane == __ffsll((long long)over) - 1) {
        uint32_t run = incl - s;
        for (int q = 0; q < per; ++q) {
            const uint32_t h = hist[lane * per + q];
            if (run + h >= need) {
                ctl->bin = (uint32_t)(lane * per + q);
                ctl->need = need - run;
                ctl->fin = run + h == need ? 1u : 0u;
                break;
            }
            run += h;
        }
    }
}

__global__ __launch_bounds__(kLanes *kBeamMaxWaves) void beam_search_kernel(
    const double *S_all, const double *D_all, int n, int W, int depot, int select_cost, int masks_in_lds, int32_t *best_tour,
    double *best_score, double *best_cost, int32_t *n_beams, int32_t *status_out, int32_t *beam_tours, double *beam_score,
    double *beam_cost, unsigned char *workspace, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & (kLanes - 1), wave = tid / kLanes, nwaves = nthr / kLanes;
    const int nw = beam_words(n);
    const size_t tlen = (size_t)n + 1;

    unsigned char *p = smem;
    BeamCtl *ctl = reinterpret_cast<BeamCtl *>(p);  p += beam_r16(sizeof(BeamCtl));
    uint32_t *hist = reinterpret_cast<uint32_t *>(p);  p += (size_t)kBins * sizeof(uint32_t);
    double *cbuf0 = reinterpret_cast<double *>(p);  p += beam_r16((size_t)W * 8);
    double *cbuf1 = reinterpret_cast<double *>(p);  p += beam_r16((size_t)W * 8);
    uint64_t *ckey = reinterpret_cast<uint64_t *>(p);  p += beam_r16((size_t)W * 8);
    int32_t *lbuf0 = reinterpret_cast<int32_t *>(p);  p += beam_r16((size_t)W * 4);
    int32_t *lbuf1 = reinterpret_cast<int32_t *>(p);  p += beam_r16((size_t)W * 4);
    uint32_t *cid = reinterpret_cast<uint32_t *>(p);  p += beam_r16((size_t)W * 4);
    uint32_t *par = hist;                                 // the sorted ids of a step: the histogram is idle then (W <= kBins)

    unsigned char *ws = workspace + (size_t)b * ws_stride;
    uint32_t *bp = reinterpret_cast<uint32_t *>(ws);
    int32_t *tours = beam_tours ? beam_tours + (size_t)b * W * tlen : reinterpret_cast<int32_t *>(ws + beam_bp_bytes(n, W));
    uint64_t *mbuf0 = masks_in_lds ? reinterpret_cast<uint64_t *>(p)
                                   : reinterpret_cast<uint64_t *>(ws + beam_bp_bytes(n, W) + beam_tours_bytes(n, W));
    uint64_t *mbuf1 = mbuf0 + (size_t)W * nw;

    const double *S = S_all + (size_t)b * n * n;
    const double *D = D_all ? D_all + (size_t)b * n * n : nullptr;
    int32_t *bt = best_tour + (size_t)b * tlen;
    double *bscore = beam_score ? beam_score + (size_t)b * W : nullptr;
    double *bcost = beam_cost ? beam_cost + (size_t)b * W : nullptr;

    // ---- refusal: an off-diagonal entry that is not finite ------------------------------------------------------------------
    if (tid == 0) ctl->bad = 0;
    __syncthreads();
    {
        bool bad = false;
        for (int q = tid; q < n * n; q += nthr) {
            const int i = q / n;
            if (q - i * n != i && !isfinite(S[q])) bad = true;
        }
        if (bad) ctl->bad = 1;
    }
    __syncthreads();
    if (ctl->bad) {
        for (int q = tid; q <= n; q += nthr) bt[q] = -1;
        if (beam_tours)
            for (size_t q = tid; q < (size_t)W * tlen; q += nthr) tours[q] = -1;
        if (bscore)
            for (int r = tid; r < W; r += nthr) { bscore[r] = NAN; bcost[r] = NAN; }
        if (tid == 0) { best_score[b] = NAN; best_cost[b] = NAN; n_beams[b] = 0; status_out[b] = kBeamStatusBadScore; }
        return;
    }

    // ---- step 0 ---------------------------------------------------------------------------------------------------------------
    int cur = 0, nb = 1;
    if (tid == 0) { cbuf0[0] = 0.0; lbuf0[0] = depot; }
    for (int q = tid; q < W; q += nthr) { ckey[q] = 0ull; cid[q] = 0u; }         // every id the sort reads names a beam and a node
    for (int w = tid; w < nw; w += nthr) mbuf0[w] = (depot / kLanes == w) ? 1ull << (depot & (kLanes - 1)) : 0ull;
    __syncthreads();

    for (int t = 1; t < n; ++t) {
        const double *c = cur ? cbuf1 : cbuf0;
        const int32_t *last = cur ? lbuf1 : lbuf0;
        const uint64_t *mask = cur ? mbuf1 : mbuf0;
        double *cn = cur ? cbuf0 : cbuf1;
        int32_t *ln = cur ? lbuf0 : lbuf1;
        uint64_t *mn = cur ? mbuf0 : mbuf1;
        const int total = nb * (n - t);
        const int nn = total < W ? total : W;

        // ---- select: the cut (T, idT): a candidate is kept iff key < T or (key == T and id <= idT) ---------------------------------
        uint64_t T = ~0ull;
        uint32_t idT = kIdAll;
        if (total > W) {
            uint64_t prefix = 0ull;
            uint32_t need = (uint32_t)W, kT = 0u;
            for (int d = 0; d < 8; ++d) {
                for (int q = tid; q < kBins; q += nthr) hist[q] = 0u;
                __syncthreads();
                const int shift = d < 5 ? 53 - 11 * d : 0;               // key digits at bits 53, 42, 31, 20, 9 (11 wide) and 0 (9 wide)
                const int hs = d < 5 ? shift + 11 : 9;                    // the digits above this one
                const uint32_t dmask = d < 5 ? 0x7FFu : 0x1FFu;
                for_candidates(S, n, nw, nb, c, last, mask, wave, nwaves, lane, [&](bool valid, uint64_t key, int k, int j) {
                    bool m;
                    uint32_t digit;
                    if (d < 6) {
                        m = valid && (hs >= 64 || (key >> hs) == (prefix >> hs));
                        digit = (uint32_t)(key >> shift) & dmask;
                    } else if (d == 6) {
                        m = valid && key == prefix;
                        digit = (uint32_t)k;
                    } else {
                        m = valid && key == prefix && (uint32_t)k == kT;
                        digit = (uint32_t)j;
                    }
                    hist_add(hist, m, digit, lane);
                });
                __syncthreads();
                if (wave == 0) find_bin(hist, need, lane, ctl);
                __syncthreads();
                const uint32_t bin = ctl->bin;
                const bool fin = ctl->fin != 0u;
                need = ctl->need;
                if (d < 6) prefix |= (uint64_t)bin << shift;
                else if (d == 6) kT = bin;
                if (fin || d == 7) {
                    if (d < 6) { T = prefix | (shift ? (1ull << shift) - 1ull : 0ull); idT = kIdAll; }
                    else if (d == 6) { T = prefix; idT = (kT << kIdBits) | ((1u << kIdBits) - 1u); }
                    else { T = prefix; idT = (kT << kIdBits) | bin; }
                    break;
                }
            }
        }

        // ---- emit ---------------------------------------------------------------------------------------------------------------
        if (tid == 0) ctl->count = 0u;
        __syncthreads();
        for_candidates(S, n, nw, nb, c, last, mask, wave, nwaves, lane, [&](bool valid, uint64_t key, int k, int j) {
            const uint32_t id = ((uint32_t)k << kIdBits) | (uint32_t)j;
            const bool sel = valid && (key < T || (key == T && id <= idT));
            const unsigned long long bm = __ballot(sel);
            if (bm == 0ull) return;
            uint32_t base = 0u;
            if (lane == 0) base = atomicAdd(&ctl->count, (uint32_t)__popcll((long long)bm));
            base = (uint32_t)__shfl((int)base, 0);
            if (sel) {
                const uint32_t pos = base + (uint32_t)__popcll((long long)(bm & ((1ull << lane) - 1ull)));
                if (pos < (uint32_t)nn) { ckey[pos] = key; cid[pos] = id; }     // always: exactly nn candidates pass the cut
            }
        });
        __syncthreads();

        // ---- sort by counting; the rank is the new beam --------------------------------------------------------------------------
        for (int i = tid; i < nn; i += nthr) {
            const uint64_t ki = ckey[i];
            const uint32_t ii = cid[i];
            int rank = 0;
            for (int m = 0; m < nn; ++m) {
                const uint64_t km = ckey[m];
                const uint32_t im = cid[m];
                rank += (km < ki || (km == ki && im < ii)) ? 1 : 0;
            }
            cn[rank] = value_of(ki);
            ln[rank] = (int32_t)(ii & ((1u << kIdBits) - 1u));
            par[rank] = ii;
            bp[(size_t)(t - 1) * W + rank] = ii;
        }
        __syncthreads();
        for (int q = tid; q < nn * nw; q += nthr) {
            const int r = q / nw, w = q - r * nw;
            const uint32_t ii = par[r];
            const int k = (int)(ii >> kIdBits), j = (int)(ii & ((1u << kIdBits) - 1u));
            uint64_t m = mask[(size_t)k * nw + w];
            if (j / kLanes == w) m |= 1ull << (j & (kLanes - 1));
            mn[q] = m;
        }
        __syncthreads();
        cur ^= 1;
        nb = nn;
    }

    // ---- close ------------------------------------------------------------------------------------------------------------------
    const double *c = cur ? cbuf1 : cbuf0;
    const int32_t *last = cur ? lbuf1 : lbuf0;
    double *fscore = cur ? cbuf0 : cbuf1;                 // the final scores; the costs go where the sort keys were
    double *fcost = reinterpret_cast<double *>(ckey);
    for (int r = tid; r < W; r += nthr) {
        double sc = NAN, co = NAN;
        if (r < nb) {
            int32_t *tr = tours + (size_t)r * tlen;
            int pr = r;
            for (int t = n - 1; t >= 1; --t) {
                const uint32_t e = bp[(size_t)(t - 1) * W + pr];
                tr[t] = (int32_t)(e & ((1u << kIdBits) - 1u));
                pr = (int)(e >> kIdBits);
            }
            tr[0] = depot;
            tr[n] = depot;
            sc = value_of(key_of(c[r], S[(size_t)last[r] * n + depot]));
            if (D) {
                co = 0.0;
                int x = depot;
                for (int q = 1; q <= n; ++q) {
                    const int y = tr[q];
                    co = co + D[(size_t)x * n + y];
                    x = y;
                }
            }
        } else if (beam_tours) {
            int32_t *tr = tours + (size_t)r * tlen;
            for (int q = 0; q <= n; ++q) tr[q] = -1;
        }
        fscore[r] = sc;
        fcost[r] = co;
        if (bscore) { bscore[r] = sc; bcost[r] = co; }
    }
    __syncthreads();
    if (wave == 0) {
        const double *v = select_cost ? fcost : fscore;
        int bi = -1;
        double bv = 0.0;
        for (int r = lane; r < nb; r += kLanes)
            if (bi < 0 || v[r] < bv) { bv = v[r]; bi = r; }
#pragma unroll
        for (int d = kLanes / 2; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(bv, d);
            const int oi = __shfl_xor(bi, d);
            if (oi >= 0 && (bi < 0 || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) ctl->best = bi;
    }
    __syncthreads();
    const int best = ctl->best;
    const int32_t *won = tours + (size_t)best * tlen;
    for (int q = tid; q <= n; q += nthr) bt[q] = won[q];
    if (tid == 0) { best_score[b] = fscore[best]; best_cost[b] = fcost[best]; n_beams[b] = nb; status_out[b] = 0; }
}

}  // namespace

bool beam_masks_in_lds(int n, int width) { return beam_fixed_lds(width) + beam_mask_bytes(n, width) <= kBeamLdsBudget; }

size_t beam_lds_bytes(int n, int width) {
    return beam_fixed_lds(width) + (beam_masks_in_lds(n, width) ? beam_mask_bytes(n, width) : 0);
}

size_t beam_workspace_bytes(int B, int n, int width) {
    const size_t per = beam_bp_bytes(n, width) + beam_tours_bytes(n, width) + (beam_masks_in_lds(n, width) ? 0 : beam_mask_bytes(n, width));
    return (size_t)B * per;
}

hipError_t launch_beam_search(const double *S, const double *D, int B, int n, int width, int depot, int select_cost, int32_t *best_tour,
                              double *best_score, double *best_cost, int32_t *n_beams, int32_t *status, int32_t *beam_tours,
                              double *beam_score, double *beam_cost, void *workspace, hipStream_t stream) {
    if (B == 0) return hipSuccess;
    const size_t lds = beam_lds_bytes(n, width);
    const int waves = width < kBeamMaxWaves ? width : kBeamMaxWaves;
    const size_t stride = beam_workspace_bytes(1, n, width);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(beam_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    (void)hipGetLastError();
    hipLaunchKernelGGL(beam_search_kernel, dim3((unsigned)B), dim3(kLanes * waves), lds, stream, S, D, n, width, depot, select_cost,
                       beam_masks_in_lds(n, width) ? 1 : 0, best_tour, best_score, best_cost, n_beams, status, beam_tours, beam_score,
                       beam_cost, static_cast<unsigned char *>(workspace), stride);
    return hipGetLastError();
}

}  // namespace gnngls
