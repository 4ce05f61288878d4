// yf_anchor_kernels.hip -- yolov5's autoanchor on the device: the ratio metric of up to 1024 candidate anchors in one pass over the label
// shapes, the evolution chain scored YF_ANCHOR_BATCH generations per pass, and a lock-step k-means on quantised labels.
// include/yolo_fastest_hip.h states the rule; every sum is an exact integer, so no result depends on the order anything runs in.
// No workgroup waits on another: sums cross workgroups as uint64 vector atomics, and the launch boundary is the exchange.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/yolo_fastest_hip.h"

namespace yf {
int set_error(int code, const char* msg);   // yf_engine.hip: the slot yf_last_error_string() reads
}

namespace {

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return yf::set_error(code, buf);
}
#define HIP_OK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(YF_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

typedef unsigned long long u64;
constexpr int ANCHOR_THREADS = 256;      // 4 waves
constexpr int ANCHOR_LPL = 4;            // labels per lane and pass of the set loop: one wave reduction per set serves 256 labels
constexpr int ANCHOR_MAX_CAND = 1024;    // S * A (metric), R * A (k-means): what the LDS tables are sized for
constexpr int ANCHOR_MAX_BLOCKS = 1024;  // the grid strides over the labels beyond this: bounds the atomics per accumulator

__device__ __forceinline__ u64 wave_sum_u64(u64 v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// x of one (label, anchor) pair: min(min(rw, 1 / rw), min(rh, 1 / rh)), four correctly rounded fp32 divisions.  No NaN can arise from a
// label in [0, 2^15) and a finite positive anchor (0 / a = 0, 1 / 0 = inf, 1 / inf = 0), so the plain comparisons are torch.min's result.
__device__ __forceinline__ float ratio_x(float w, float h, float aw, float ah)
{
    const float rw = w / aw, rh = h / ah;
    const float iw = 1.0f / rw, ih = 1.0f / rh;
    const float mw = iw < rw ? iw : rw, mh = ih < rh ? ih : rh;
    return mh < mw ? mh : mw;
}

// out uint64 [S,3] += (fit, cnt_best, cnt_x) of this workgroup's labels; out is zeroed by the launcher.  One label per lane, ANCHOR_LPL
// of them in registers; the S * A candidates sit in LDS and are read as broadcasts.
__global__ __launch_bounds__(ANCHOR_THREADS) void anchor_metric_kernel(const float2* __restrict__ wh, int n, const float2* __restrict__ anchors,
                                                                       int S, int A, float t, float scale, u64* __restrict__ out)
{
    __shared__ float2 s_anc[ANCHOR_MAX_CAND];
    __shared__ u64 s_acc[3 * ANCHOR_MAX_CAND];                          // S <= 1024 (A = 1): 24 KB beside the candidates' 8 KB
    for (int i = threadIdx.x; i < S * A; i += ANCHOR_THREADS) s_anc[i] = anchors[i];
    for (int i = threadIdx.x; i < 3 * S; i += ANCHOR_THREADS) s_acc[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (long base = (long)blockIdx.x * (ANCHOR_THREADS * ANCHOR_LPL); base < n; base += (long)gridDim.x * (ANCHOR_THREADS * ANCHOR_LPL)) {
        float2 l[ANCHOR_LPL];
#pragma unroll
        for (int j = 0; j < ANCHOR_LPL; ++j) {
            const long i = base + j * ANCHOR_THREADS + threadIdx.x;
            l[j] = i < n ? wh[i] : make_float2(0.0f, 0.0f);             // (0, 0): x = 0 against every anchor, counted nowhere (t > 0)
        }
        for (int s = 0; s < S; ++s) {
            const float2* anc = s_anc + s * A;
            u64 fit = 0;
            unsigned cnt = 0;                                           // cnt_x | cnt_best << 16: a wave's 256 labels give <= 8192 and <= 256
#pragma unroll
            for (int j = 0; j < ANCHOR_LPL; ++j) {
                float best = 0.0f;
                for (int a = 0; a < A; ++a) {
                    const float2 k = anc[a];
                    const float x = ratio_x(l[j].x, l[j].y, k.x, k.y);
                    cnt += x > t ? 1u : 0u;
                    best = x > best ? x : best;
                }
                if (best > t) {                                         // best >= 2^-m: a multiple of 2^-(23+m), the product an exact integer <= 2^31
                    fit += (u64)(unsigned)(best * scale);
                    cnt += 1u << 16;
                }
            }
            fit = wave_sum_u64(fit);
            cnt = wave_sum_u32(cnt);
            if (lane == 0 && cnt) {
                atomicAdd(&s_acc[3 * s + 0], fit);
                atomicAdd(&s_acc[3 * s + 1], (u64)(cnt >> 16));
                atomicAdd(&s_acc[3 * s + 2], (u64)(cnt & 0xffffu));
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * S; i += ANCHOR_THREADS)
        if (s_acc[i]) atomicAdd(&out[i], s_acc[i]);
}

void launch_anchor_metric(const float* wh, int n, const float* anchors, int S, int A, float t, int m, u64* out, hipStream_t s)
{
    const long per = ANCHOR_THREADS * ANCHOR_LPL;
    const int grid = (int)std::min<long>((n + per - 1) / per, ANCHOR_MAX_BLOCKS);
    anchor_metric_kernel<<<grid, ANCHOR_THREADS, 0, s>>>((const float2*)wh, n, (const float2*)anchors, S, A, t, ldexpf(1.0f, 23 + m), out);
}

// t = (float)(1.0 / thr) and m = the smallest integer with 2^-m <= t
void threshold_of(double thr, float* t, int* m)
{
    *t = (float)(1.0 / thr);
    int mm = 0;
    while (ldexpf(1.0f, -mm) > *t) ++mm;
    *m = mm;
}

// ---- k-means ----
// cent double [R,A,2] = the observations of the label rows init[r][a]
__global__ void kmeans_init_kernel(const int32_t* __restrict__ q, const int32_t* __restrict__ init, int RA, double s_w, double s_h,
                                   double* __restrict__ cent)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= RA) return;
    const long row = init[i];
    cent[2 * i + 0] = ((double)q[2 * row + 0] / 64.0) / s_w;
    cent[2 * i + 1] = ((double)q[2 * row + 1] / 64.0) / s_h;
}

// sums uint64 [R,A,3] += (sum q_w, sum q_h, count) of the labels nearest to each centroid; zeroed by the launcher.  Dynamic LDS:
// R * A * (2 doubles + 3 uint64).  One label per lane; the LDS atomics of a wave collide where its labels share a cluster.
__global__ __launch_bounds__(ANCHOR_THREADS) void kmeans_assign_kernel(const int2* __restrict__ q, int n, const double* __restrict__ cent, int R, int A,
                                                                       double s_w, double s_h, u64* __restrict__ sums)
{
    extern __shared__ double s_dyn[];
    double* s_cent = s_dyn;
    u64* s_sum = (u64*)(s_dyn + 2 * R * A);
    for (int i = threadIdx.x; i < 2 * R * A; i += ANCHOR_THREADS) s_cent[i] = cent[i];
    for (int i = threadIdx.x; i < 3 * R * A; i += ANCHOR_THREADS) s_sum[i] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * ANCHOR_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * ANCHOR_THREADS) {
        const int2 l = q[i];
        const double ow = ((double)l.x / 64.0) / s_w, oh = ((double)l.y / 64.0) / s_h;
        for (int r = 0; r < R; ++r) {
            const double* c = s_cent + 2 * r * A;
            int arg = 0;
            double dmin = 0.0;
            for (int a = 0; a < A; ++a) {
                const double dw = ow - c[2 * a], dh = oh - c[2 * a + 1];
                const double d = dw * dw + dh * dh;
                if (a == 0 || d < dmin) {                      // strict: the lowest index on ties
                    dmin = d;
                    arg = a;
                }
            }
            u64* acc = s_sum + 3 * (r * A + arg);
            atomicAdd(acc + 0, (u64)l.x);
            atomicAdd(acc + 1, (u64)l.y);
            atomicAdd(acc + 2, (u64)1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * R * A; i += ANCHOR_THREADS)
        if (s_sum[i]) atomicAdd(&sums[i], s_sum[i]);
}

bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

int check_common(const char* who, int n, int A, int sets, const char* sets_name, double thr)
{
    if (n < 1) return fail(YF_E_INVALID, "%s: n >= 1", who);
    if (A < 1 || A > YF_ANCHOR_MAX_A) return fail(YF_E_INVALID, "%s: 1 <= A <= %d", who, YF_ANCHOR_MAX_A);
    if (sets < 1 || (long)sets * A > ANCHOR_MAX_CAND) return fail(YF_E_INVALID, "%s: %s >= 1 and %s * A <= %d", who, sets_name, sets_name, ANCHOR_MAX_CAND);
    if (!(thr >= 1.0 && thr <= 256.0)) return fail(YF_E_INVALID, "%s: thr must be in [1, 256] (and not NaN)", who);
    return YF_OK;
}

// work layouts (bytes); every piece 8-byte aligned
size_t evolve_work_bytes(int A) { return (size_t)YF_ANCHOR_BATCH * A * 8 + (size_t)YF_ANCHOR_BATCH * 24; }
size_t kmeans_work_bytes(int R, int A) { return (size_t)R * A * (16 + 24 + 8 + 4) + (size_t)R * 24 + 8; }

}  // namespace

extern "C" {

int yf_anchor_check_host(const float* wh, int n, const float* anchors, int num_anchors)
{
    if (n < 0 || num_anchors < 0 || (n > 0 && !wh) || (num_anchors > 0 && !anchors))
        return fail(YF_E_INVALID, "yf_anchor_check_host: null pointer or negative count");
    for (long i = 0; i < 2L * n; ++i)
        if (!(wh[i] >= 0.0f && wh[i] < 32768.0f))
            return fail(YF_E_INVALID, "yf_anchor_check_host: label %ld has a side %g: negative, not finite or >= 2^15", i / 2, (double)wh[i]);
    for (long i = 0; i < 2L * num_anchors; ++i)
        if (!finite_pos(anchors[i]))
            return fail(YF_E_INVALID, "yf_anchor_check_host: anchor %ld has a side %g: not finite and positive", i / 2, (double)anchors[i]);
    return YF_OK;
}

int yf_anchor_metric(int device, const float* d_wh, int n, const float* d_anchors, int S, int A, double thr, uint64_t* d_out, void* stream)
{
    if (!d_wh || !d_anchors || !d_out) return fail(YF_E_INVALID, "yf_anchor_metric: null pointer");
    if (int rc = check_common("yf_anchor_metric", n, A, S, "S", thr)) return rc;
    float t;
    int m;
    threshold_of(thr, &t, &m);
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipMemsetAsync(d_out, 0, (size_t)S * 24, (hipStream_t)stream));
    launch_anchor_metric(d_wh, n, d_anchors, S, A, t, m, (u64*)d_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

size_t yf_anchor_evolve_work_bytes(int A)
{
    return A < 1 || A > YF_ANCHOR_MAX_A ? 0 : evolve_work_bytes(A);
}

int yf_anchor_evolve(int device, const float* d_wh, int n, const double* k0, const double* v, int A, int gen, double thr, void* d_work,
                     size_t work_bytes, double* k_out, uint64_t* fit_out, int32_t* accepted_out, void* stream)
{
    if (!d_wh || !k0 || !v || !d_work || !k_out || !fit_out) return fail(YF_E_INVALID, "yf_anchor_evolve: null pointer");
    if (int rc = check_common("yf_anchor_evolve", n, A, YF_ANCHOR_BATCH, "YF_ANCHOR_BATCH", thr)) return rc;
    if (gen < 1) return fail(YF_E_INVALID, "yf_anchor_evolve: gen >= 1");
    if (work_bytes < evolve_work_bytes(A)) return fail(YF_E_WORKSPACE, "yf_anchor_evolve: work_bytes %zu < %zu", work_bytes, evolve_work_bytes(A));
    for (int i = 0; i < 2 * A; ++i)
        if (!finite_pos(k0[i])) return fail(YF_E_INVALID, "yf_anchor_evolve: anchor %d has a side %g: not finite and positive", i / 2, k0[i]);
    for (long i = 0; i < 2L * A * gen; ++i)
        if (!std::isfinite(v[i])) return fail(YF_E_INVALID, "yf_anchor_evolve: mutation factor %ld is not finite", i);
    float t;
    int m;
    threshold_of(thr, &t, &m);
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipSetDevice(device));
    float* d_cand = (float*)d_work;                                               // [G,A,2]
    u64* d_sums = (u64*)((char*)d_work + (size_t)YF_ANCHOR_BATCH * A * 8);         // [G,3]
    std::vector<double> k(k0, k0 + 2 * A), kg((size_t)YF_ANCHOR_BATCH * 2 * A);
    std::vector<float> cand((size_t)YF_ANCHOR_BATCH * 2 * A);
    std::vector<u64> sums((size_t)YF_ANCHOR_BATCH * 3);
    // one pass: the candidates up, one launch, the sums down, one synchronisation
    auto pass = [&](int S) -> int {
        HIP_OK(hipMemcpyAsync(d_cand, cand.data(), (size_t)S * A * 8, hipMemcpyHostToDevice, s));
        HIP_OK(hipMemsetAsync(d_sums, 0, (size_t)S * 24, s));
        launch_anchor_metric(d_wh, n, d_cand, S, A, t, m, d_sums, s);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(sums.data(), d_sums, (size_t)S * 24, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        return YF_OK;
    };
    for (int i = 0; i < 2 * A; ++i) cand[i] = (float)k[i];
    if (int rc = pass(1)) return rc;
    u64 f = sums[0];
    for (int g = 0; g < gen; ++g)
        if (accepted_out) accepted_out[g] = 0;
    for (int g0 = 0; g0 < gen;) {
        const int S = std::min((int)YF_ANCHOR_BATCH, gen - g0);
        for (int j = 0; j < S; ++j)
            for (int i = 0; i < 2 * A; ++i) {
                const double x = k[i] * v[(size_t)(g0 + j) * 2 * A + i];
                kg[(size_t)j * 2 * A + i] = x < 2.0 ? 2.0 : x;                     // numpy's clip(min=2.0)
                cand[(size_t)j * 2 * A + i] = (float)kg[(size_t)j * 2 * A + i];
            }
        if (int rc = pass(S)) return rc;
        int hit = -1;
        for (int j = 0; j < S && hit < 0; ++j)
            if (sums[3 * j] > f) hit = j;          // the first improvement only: the generations behind it meet the new k in the next pass
        if (hit < 0) {
            g0 += S;
            continue;
        }
        f = sums[3 * hit];
        for (int i = 0; i < 2 * A; ++i) k[i] = kg[(size_t)hit * 2 * A + i];
        if (accepted_out) accepted_out[g0 + hit] = 1;
        g0 += hit + 1;
    }
    memcpy(k_out, k.data(), sizeof(double) * 2 * A);
    *fit_out = f;
    return YF_OK;
}

size_t yf_anchor_kmeans_work_bytes(int R, int A)
{
    return R < 1 || A < 1 || A > YF_ANCHOR_MAX_A || (long)R * A > ANCHOR_MAX_CAND ? 0 : kmeans_work_bytes(R, A);
}

int yf_anchor_kmeans(int device, const int32_t* d_q, int n, const double* s, const int32_t* init, int R, int A, int max_iter, double thr,
                     const float* d_wh, void* d_work, size_t work_bytes, double* k_out, int32_t* winner_out, int32_t* iters_out, void* stream)
{
    if (!d_q || !s || !init || !d_wh || !d_work || !k_out || !winner_out || !iters_out) return fail(YF_E_INVALID, "yf_anchor_kmeans: null pointer");
    if (int rc = check_common("yf_anchor_kmeans", n, A, R, "R", thr)) return rc;
    if (max_iter < 1) return fail(YF_E_INVALID, "yf_anchor_kmeans: max_iter >= 1");
    if (!finite_pos(s[0]) || !finite_pos(s[1])) return fail(YF_E_INVALID, "yf_anchor_kmeans: s must be finite and positive");
    for (int i = 0; i < R * A; ++i)
        if (init[i] < 0 || init[i] >= n) return fail(YF_E_INVALID, "yf_anchor_kmeans: init[%d] = %d is not a label row", i, init[i]);
    if (work_bytes < kmeans_work_bytes(R, A)) return fail(YF_E_WORKSPACE, "yf_anchor_kmeans: work_bytes %zu < %zu", work_bytes, kmeans_work_bytes(R, A));
    float t;
    int m;
    threshold_of(thr, &t, &m);
    hipStream_t st = (hipStream_t)stream;
    HIP_OK(hipSetDevice(device));
    const int RA = R * A;
    char* w = (char*)d_work;
    double* d_cent = (double*)w;               w += (size_t)RA * 16;      // [R,A,2]
    u64* d_sums = (u64*)w;                     w += (size_t)RA * 24;      // [R,A,3]
    float* d_cand = (float*)w;                 w += (size_t)RA * 8;       // [R,A,2]: the survivors' de-whitened centroids
    u64* d_fit = (u64*)w;                      w += (size_t)R * 24;       // [R,3]
    int32_t* d_init = (int32_t*)w;                                        // [R,A]
    HIP_OK(hipMemcpyAsync(d_init, init, (size_t)RA * 4, hipMemcpyHostToDevice, st));
    kmeans_init_kernel<<<(RA + 255) / 256, 256, 0, st>>>(d_q, d_init, RA, s[0], s[1], d_cent);
    HIP_OK(hipGetLastError());
    std::vector<int> active(R);                                            // restarts still iterating, ascending: slot i of the device tables
    for (int r = 0; r < R; ++r) {
        active[r] = r;
        iters_out[r] = 0;
    }
    std::vector<u64> prev((size_t)RA * 3), got((size_t)RA * 3);
    std::vector<char> has_prev(R, 0);
    std::vector<double> cent((size_t)RA * 2), up((size_t)RA * 2);          // cent: every restart's latest centroids, whitened
    const int grid = (int)std::min<long>(((long)n + ANCHOR_THREADS - 1) / ANCHOR_THREADS, 256);
    for (int it = 1; it <= max_iter && !active.empty(); ++it) {
        const int Ra = (int)active.size();
        HIP_OK(hipMemsetAsync(d_sums, 0, (size_t)Ra * A * 24, st));
        kmeans_assign_kernel<<<grid, ANCHOR_THREADS, (size_t)Ra * A * 40, st>>>((const int2*)d_q, n, d_cent, Ra, A, s[0], s[1], d_sums);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(got.data(), d_sums, (size_t)Ra * A * 24, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        std::vector<int> next;
        for (int i = 0; i < Ra; ++i) {
            const int r = active[i];
            const u64* g = got.data() + (size_t)i * A * 3;
            u64* p = prev.data() + (size_t)r * A * 3;
            bool empty = false;
            for (int a = 0; a < A; ++a) empty |= g[3 * a + 2] == 0;
            if (empty) {
                iters_out[r] = -1;
                continue;
            }
            iters_out[r] = it;
            const bool same = has_prev[r] && memcmp(g, p, sizeof(u64) * 3 * A) == 0;
            memcpy(p, g, sizeof(u64) * 3 * A);
            has_prev[r] = 1;
            for (int a = 0; a < A; ++a)
                for (int c = 0; c < 2; ++c)
                    cent[((size_t)r * A + a) * 2 + c] = ((double)g[3 * a + c] / (64.0 * (double)g[3 * a + 2])) / s[c];
            if (!same && it < max_iter) next.push_back(r);
        }
        active.swap(next);
        if (!active.empty() && it < max_iter) {
            for (size_t i = 0; i < active.size(); ++i) memcpy(up.data() + i * A * 2, cent.data() + (size_t)active[i] * A * 2, sizeof(double) * 2 * A);
            HIP_OK(hipMemcpyAsync(d_cent, up.data(), active.size() * A * 16, hipMemcpyHostToDevice, st));
            HIP_OK(hipStreamSynchronize(st));                              // `up` is rewritten next round
        }
    }
    // the survivors' fitness in one launch; a survivor whose de-whitened centroids are not finite and positive as floats is discarded too
    std::vector<int> surv;
    std::vector<float> cand;
    for (int r = 0; r < R; ++r) {
        if (iters_out[r] < 0) continue;
        bool ok = true;
        for (int i = 0; i < 2 * A; ++i) ok &= finite_pos((double)(float)(cent[(size_t)r * A * 2 + i] * s[i & 1]));
        if (!ok) {
            iters_out[r] = -1;
            continue;
        }
        surv.push_back(r);
        for (int i = 0; i < 2 * A; ++i) cand.push_back((float)(cent[(size_t)r * A * 2 + i] * s[i & 1]));
    }
    *winner_out = -1;
    if (surv.empty()) return YF_OK;
    std::vector<u64> fit(surv.size() * 3);
    HIP_OK(hipMemcpyAsync(d_cand, cand.data(), cand.size() * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_fit, 0, surv.size() * 24, st));
    launch_anchor_metric(d_wh, n, d_cand, (int)surv.size(), A, t, m, d_fit, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(fit.data(), d_fit, surv.size() * 24, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    size_t best = 0;
    for (size_t i = 1; i < surv.size(); ++i)
        if (fit[3 * i] > fit[3 * best]) best = i;                          // strict: the earliest restart on ties
    *winner_out = surv[best];
    for (int i = 0; i < 2 * A; ++i) k_out[i] = cent[(size_t)surv[best] * A * 2 + i] * s[i & 1];
    return YF_OK;
}

}  // extern "C"
