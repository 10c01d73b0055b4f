// labels_kernels.hip -- regret labels of the training data (datasets.py:23-34, scripts/generate_instances.py:17-20) on gfx950.
//
// The fixed-edge searches themselves run on the persistent search kernel (gls_kernels.hip) unchanged: capi.hip's
// gnngls_regret_labels expands a chunk of jobs into per-job matrices D' here, runs gnngls_gls_run on them with D' as the
// guide, and collects the labels here.  See labels_kernels.h for the definition of a job.
#include "labels_kernels.h"

#include "gls_kernels.h"

namespace gnngls {

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) label_offsets_kernel(const double *D, int n, double *offset) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x;
    const double *d = D + (size_t)b * n * n;
    double m = -__builtin_inf();
    for (int q = threadIdx.x; q < n * n; q += kThreads) m = fmax(m, d[q]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // one rounding (a product, nothing to contract), then exact: frexp / ldexp -- gnngls_amd.labels.fixed_edge_offset
        // computes the same value on the host
        const double x = (2.0 * n) * red[0];
        double M = 1.0;
        if (x > 0.0 && x < __builtin_inf()) {
            int e;
            const double f = frexp(x, &e);
            M = f == 0.5 ? x : ldexp(1.0, e);
        }
        offset[b] = M;
    }
}

__global__ void __launch_bounds__(kThreads) label_init_kernel(int n, int N, const int32_t *base_tour, int keep_edge_cost,
                                                              double *edge_cost, const double *base_cost, double *best_cost,
                                                              int32_t *best_rank, int32_t *best_tour, int32_t *status) {
    const int b = blockIdx.x;
    for (int p = threadIdx.x; p <= n; p += kThreads) best_tour[(size_t)b * (n + 1) + p] = base_tour[(size_t)b * (n + 1) + p];
    if (!keep_edge_cost)
        for (int r = threadIdx.x; r < N; r += kThreads) edge_cost[(size_t)b * N + r] = __builtin_inf();
    if (threadIdx.x == 0) {
        best_cost[b] = base_cost[b];
        best_rank[b] = -1;
        status[b] = 0;
    }
}

// one workgroup per job: D' = D_inst with the two entries of the fixed edge lowered by M_inst; start tour = the base tour
__global__ void __launch_bounds__(kThreads) label_expand_kernel(const double *D, int n, const int32_t *base_tour, const LabelJob *jobs,
                                                                const double *offset, double *Dp, int32_t *tours) {
    const LabelJob jb = jobs[blockIdx.x];
    const double *d = D + (size_t)jb.inst * n * n;
    double *dp = Dp + (size_t)blockIdx.x * n * n;
    const double M = offset[jb.inst];
    const int q1 = jb.i * n + jb.j, q2 = jb.j * n + jb.i;
    for (int q = threadIdx.x; q < n * n; q += kThreads) {
        double v = d[q];
        if (q == q1 || q == q2) v = v - M;
        dp[q] = v;
    }
    for (int p = threadIdx.x; p <= n; p += kThreads)
        tours[(size_t)blockIdx.x * (n + 1) + p] = base_tour[(size_t)jb.inst * (n + 1) + p];
}

// one thread per job: the label (tour_cost of the returned tour on the instance's own D, summed in tour order like
// gnngls/__init__.py:17-21) and the check that the tour holds the fixed edge
__global__ void label_cost_kernel(const double *D, int n, int N, const LabelJob *jobs, int J, const int32_t *tours,
                                  const int32_t *job_status, double *job_cost, double *edge_cost, int32_t *status) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= J) return;
    const LabelJob jb = jobs[k];
    const int st = job_status[k];
    if (st == GNNGLS_STATUS_PENALTY_OVERFLOW_DEV) {            // rerun by the caller with 32-bit counters
        job_cost[k] = __builtin_nan("");
        return;
    }
    const int32_t *t = tours + (size_t)k * (n + 1);
    const double *d = D + (size_t)jb.inst * n * n;
    double c = 0.0;
    bool has = false;
    for (int p = 0; p < n; ++p) {
        const int a = t[p], e = t[p + 1];
        c += d[(size_t)a * n + e];
        has |= (a == jb.i && e == jb.j) || (a == jb.j && e == jb.i);
    }
    if (!has) {
        atomicMax(&status[jb.inst], GNNGLS_STATUS_EDGE_LOST_DEV);
        job_cost[k] = __builtin_nan("");
        return;
    }
    if (st != 0) atomicMax(&status[jb.inst], st);
    job_cost[k] = c;
    double *ec = edge_cost + (size_t)jb.inst * N + jb.r;        // one job per (instance, edge) in a launch: no race
    if (c < *ec) *ec = c;
}

// the jobs of an instance are contiguous in a chunk: the thread of its first job takes the lexicographic minimum of
// (cost, rank) over them and the current best (the base tour has rank -1) -- the same winner whatever the chunking
__global__ void label_best_kernel(int n, const LabelJob *jobs, int J, const int32_t *tours, const double *job_cost,
                                  double *best_cost, int32_t *best_rank, int32_t *best_tour) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= J) return;
    const int inst = jobs[k].inst;
    if (k > 0 && jobs[k - 1].inst == inst) return;
    double bc = best_cost[inst];
    int br = best_rank[inst], arg = -1;
    for (int q = k; q < J && jobs[q].inst == inst; ++q) {
        const double c = job_cost[q];                           // NaN (skipped or lost) never wins
        const int r = jobs[q].r;
        if (c < bc || (c == bc && r < br)) { bc = c; br = r; arg = q; }
    }
    if (arg < 0) return;
    best_cost[inst] = bc;
    best_rank[inst] = br;
    for (int p = 0; p <= n; ++p) best_tour[(size_t)inst * (n + 1) + p] = tours[(size_t)arg * (n + 1) + p];
}

__global__ void __launch_bounds__(kThreads) label_finalize_kernel(int n, int N, const int32_t *base_tour, const double *base_cost,
                                                                  double *edge_cost, double *regret) {
    __shared__ int pos[256];
    const int b = blockIdx.x;
    const int32_t *t = base_tour + (size_t)b * (n + 1);
    for (int p = threadIdx.x; p < n; p += kThreads) pos[t[p]] = p;
    __syncthreads();
    const double bc = base_cost[b];
    for (int q = threadIdx.x; q < n * n; q += kThreads) {
        const int i = q / n, j = q - i * n;
        if (i >= j) continue;
        const int r = edge_rank(i, j, n);
        const int gap = abs(pos[i] - pos[j]);
        double *ec = edge_cost + (size_t)b * N + r;
        if (gap == 1 || gap == n - 1) {
            *ec = bc;
            regret[(size_t)b * N + r] = 0.0;
        } else {
            regret[(size_t)b * N + r] = (*ec - bc) / bc;        // datasets.py:31
        }
    }
}

}  // namespace

hipError_t launch_label_offsets(const double *D, int B, int n, double *offset, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(label_offsets_kernel, dim3(B), dim3(kThreads), 0, stream, D, n, offset);
    return hipGetLastError();
}

hipError_t launch_label_init(int B, int n, const int32_t *base_tour, const double *base_cost, bool keep_edge_cost,
                             double *edge_cost, double *best_cost, int32_t *best_rank, int32_t *best_tour, int32_t *status,
                             hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(label_init_kernel, dim3(B), dim3(kThreads), 0, stream, n, n * (n - 1) / 2, base_tour, (int)keep_edge_cost,
                       edge_cost, base_cost, best_cost, best_rank, best_tour, status);
    return hipGetLastError();
}

hipError_t launch_label_expand(const double *D, int n, const int32_t *base_tour, const LabelJob *jobs, int J, const double *offset,
                               double *Dp, int32_t *tours, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(label_expand_kernel, dim3(J), dim3(kThreads), 0, stream, D, n, base_tour, jobs, offset, Dp, tours);
    return hipGetLastError();
}

hipError_t launch_label_collect(const double *D, int n, const LabelJob *jobs, int J, const int32_t *tours, const int32_t *job_status,
                                double *job_cost, double *edge_cost, double *best_cost, int32_t *best_rank, int32_t *best_tour,
                                int32_t *status, hipStream_t stream) {
    (void)hipGetLastError();
    const int blocks = (J + 63) / 64;
    hipLaunchKernelGGL(label_cost_kernel, dim3(blocks), dim3(64), 0, stream, D, n, n * (n - 1) / 2, jobs, J, tours, job_status,
                       job_cost, edge_cost, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(label_best_kernel, dim3(blocks), dim3(64), 0, stream, n, jobs, J, tours, job_cost, best_cost, best_rank,
                       best_tour);
    return hipGetLastError();
}

hipError_t launch_label_finalize(int B, int n, const int32_t *base_tour, const double *base_cost, double *edge_cost, double *regret,
                                 hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(label_finalize_kernel, dim3(B), dim3(kThreads), 0, stream, n, n * (n - 1) / 2, base_tour, base_cost, edge_cost,
                       regret);
    return hipGetLastError();
}

}  // namespace gnngls
