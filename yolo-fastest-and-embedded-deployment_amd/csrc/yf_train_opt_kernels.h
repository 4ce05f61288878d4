// yf_train_opt_kernels.h -- sums of split partial results, channel sums (bias gradients), add / slice, Adam, SGD, ModelEMA
// Part of the training-step operators: yf_train_kernels.hip includes the family headers into ONE translation unit, INSIDE namespace yf, so the
// kernels keep their internal linkage and the launchers in that file see all of them.  Device code: include from there only.
#pragma once

// dw[i] = sum over the slabs, in slab order (deterministic).  One wave per 64 / SPL outputs: SPL lanes share an output when there are many slabs.
__global__ void __launch_bounds__(256) tsum_partials_kernel(const float* __restrict__ part, int nsplit, long nw, long part_stride,
                                                            float* __restrict__ dw, int spl)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = t / spl;
    const int j = (int)(t - i * spl);
    float v = 0.f;
    if (i < nw) {
        int sidx = j;
        for (; sidx + 3 * spl < nsplit; sidx += 4 * spl) {                // four slabs requested at once, added in slab order
            const float p0 = part[(long)sidx * part_stride + i], p1 = part[(long)(sidx + spl) * part_stride + i];
            const float p2 = part[(long)(sidx + 2 * spl) * part_stride + i], p3 = part[(long)(sidx + 3 * spl) * part_stride + i];
            v += p0; v += p1; v += p2; v += p3;
        }
        for (; sidx < nsplit; sidx += spl) v += part[(long)sidx * part_stride + i];
    }
    for (int o = spl >> 1; o > 0; o >>= 1) v += __shfl_down(v, o);       // spl is a power of two <= 64: the lanes of one output are adjacent
    if (i < nw && j == 0) dw[i] = v;
}

// per-channel sum over N, H, W (bias gradient of the head convs)
__global__ void __launch_bounds__(256) tchan_sum_kernel(const float* __restrict__ dy, int N, int C, long HW, float* __restrict__ out)
{
    __shared__ double r1[4];
    const int c = blockIdx.x;
    const long upn = (HW + 255) / 256, U = (long)N * upn;
    double s = 0;
    for (long u = 0; u < U; ++u) {
        const long n = u / upn, i = (u - n * upn) * 256 + threadIdx.x;
        if (i < HW) s += dy[(n * C + c) * HW + i];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) r1[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] = (float)(r1[0] + r1[1] + r1[2] + r1[3]);
}

// the same sum split over chunks of the (frame, pixel) list: partial sums in double to the scratch, added in chunk order by a second launch
__global__ void __launch_bounds__(256) tchan_sum_part_kernel(const float* __restrict__ dy, int N, int C, long HW, double* __restrict__ part)
{
    __shared__ double r1[4];
    const int c = blockIdx.y, nchunk = gridDim.x;
    const long hw4 = HW / 4, U = (long)N * hw4;                       // float4 units (HW % 4 == 0)
    double s = 0;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < U; u += (long)nchunk * 256) {
        const long n = u / hw4, i = (u - n * hw4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(dy + (n * C + c) * HW + i);
        s += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) r1[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)c * nchunk + blockIdx.x] = r1[0] + r1[1] + r1[2] + r1[3];
}
__global__ void tchan_sum_final_kernel(const double* __restrict__ part, int nchunk, int C, float* __restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0;
    for (int k = 0; k < nchunk; ++k) s += part[(long)c * nchunk + k];
    out[c] = (float)s;
}

// out = a + b (residual add, gradient accumulation); out may alias a
__global__ void __launch_bounds__(256) tadd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long total)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < total) out[idx] = a[idx] + b[idx];
}

// channel slices of NCHW tensors: dst[n, dc0 + c, :, :] = src[n, sc0 + c, :, :] for c < C (torch.cat over channels and its backward)
__global__ void __launch_bounds__(256) tslice_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int C, long HW, int Cs, int sc0,
                                                     int Cd, int dc0)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, total = (long)N * C * HW;
    if (idx >= total) return;
    const long i = idx % HW, c = (idx / HW) % C, n = idx / (HW * C);
    dst[(n * Cd + dc0 + c) * HW + i] = src[(n * Cs + sc0 + c) * HW + i];
}

// ---- the multi-tensor launches: training.SGD, training.Adam, training.ModelEMA and the older yf_train_adam_* entries ----
// Every tensor of a launch is one entry of a pointer table in device memory; a workgroup lies inside one tensor and finds it by bisection
// over the entries' first workgroup.  The four entry forms differ in what a tensor carries, and each size is part of the C ABI (callers
// allocate the table by it): state 1 / state 2 are Adam's exp_avg / exp_avg_sq, or SGD's momentum buffer and nothing.
struct TAdamEntry { float* p; const float* g; float* s1; float* s2; long block0; long n; };                                    // 48: yf_train_adam_multi*
struct TOptEntry { float* p; const float* g; float* s1; float* s2; long block0; long n; int group; int first; };               // 56: + param group, first step
struct TOptEmaEntry { float* p; const float* g; float* s1; float* s2; float* ema; long block0; long n; int group; int first; };    // 64: + the EMA pointer
struct TEmaEntry { const float* src; float* ema; long block0; long n; };                                                       // 32: the average alone

// The groups' scalars are kernel arguments, indexed by the entry's group (wave-uniform), so an lr edit between two steps changes no
// device memory.
enum { TOPT_MAX_GROUPS = 8, TOPT_NESTEROV = 1, TOPT_DECAY = 2, TOPT_MOMENTUM = 4 };
struct TSgdGroup { float wd, mom, neg_lr; int flags; };
struct TSgdGroups { TSgdGroup g[TOPT_MAX_GROUPS]; };
struct TAdamGroup { float wd, w1, b2, w2, eps, step_size, bc2_sqrt; int flags; };
struct TAdamGroups { TAdamGroup g[TOPT_MAX_GROUPS]; };

// What every multi-tensor kernel starts with: the tensor this workgroup belongs to, its element, the guard of the tensor's last
// workgroup; then f(entry, element).
template <class E, class F> __device__ __forceinline__ void tmulti_each(const E* __restrict__ tab, int nt, F f)
{
    int lo = 0, hi = nt - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].block0 <= (long)blockIdx.x) lo = mid; else hi = mid - 1; }
    const E e = tab[lo];
    const long idx = ((long)blockIdx.x - e.block0) * 256 + threadIdx.x;
    if (idx < e.n) f(e, idx);
}

// torch.optim.SGD(momentum, weight_decay, nesterov; dampening 0), bit for bit (the operations of torch's _single_tensor_sgd, each
// `add(x, alpha=a)` one fused multiply-add, `buf.mul_(momentum)` a rounded product of its own):
//   d = g + wd p;  buf = mom buf + d (first step: buf = d);  d = nesterov ? d + mom buf : buf;  p += -lr d
// The wd == 0 and first-step branches keep signed zeros: fma(0, p, -0.0) and 0 * mom + (-0.0) are +0.0 where torch keeps -0.0.
// Returns the parameter value it stored (the EMA goes on with it).
template <class E> __device__ __forceinline__ float tsgd_update(const E& e, const TSgdGroup& s, long idx)
{
    const float pi = e.p[idx];
    float d = e.g[idx];
    if (s.flags & TOPT_DECAY) d = __fmaf_rn(s.wd, pi, d);
    if (s.flags & TOPT_MOMENTUM) {
        float buf = d;
        if (!e.first) { const float mb = s.mom * e.s1[idx]; buf = mb + d; }
        e.s1[idx] = buf;
        d = (s.flags & TOPT_NESTEROV) ? __fmaf_rn(s.mom, buf, d) : buf;
    }
    const float pn = __fmaf_rn(s.neg_lr, d, pi);
    e.p[idx] = pn;
    return pn;
}

// torch.optim.Adam (no amsgrad), in the operation order of torch's single-tensor implementation:
//   m += (1 - b1) (g - m);  v = v b2 + (1 - b2) g g;  p += -(lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
// with weight_decay (L2, not AdamW) the gradient first becomes g + wd p, one fused multiply-add.  The scalars are formed in double on the
// host and rounded once to float, like torch's Python-double scalars (yf_train_kernels.hip: adam_groups).  The only place Adam's
// arithmetic is written: every entry point's kernel calls it.  Returns the parameter value it stored.
template <class E> __device__ __forceinline__ float tadam_update(const E& e, const TAdamGroup& s, long idx)
{
    float gi = e.g[idx];
    if (s.flags & TOPT_DECAY) gi = __fmaf_rn(s.wd, e.p[idx], gi);
    const float mi = e.s1[idx] + s.w1 * (gi - e.s1[idx]);
    const float vi = e.s2[idx] * s.b2 + (s.w2 * gi) * gi;
    e.s1[idx] = mi; e.s2[idx] = vi;
    const float pn = e.p[idx] + -s.step_size * (mi / (sqrtf(vi) / s.bc2_sqrt + s.eps));
    e.p[idx] = pn;
    return pn;
}

// yolov5's ModelEMA (training.ModelEMA): e = e d + (1 - d) p, torch's `v *= d; v += (1 - d) * p` on float32 tensors.  Three separately
// rounded operations, never contracted into a fused multiply-add (the intrinsics hold that whatever the build's -ffp-contract says);
// d and 1 - d are formed in double on the host and rounded once each, and travel as kernel arguments.
__device__ __forceinline__ float tema_update(float e, float p, float d, float omd) { return __fadd_rn(__fmul_rn(e, d), __fmul_rn(omd, p)); }

// One launch for every tensor of every param group: the update the group type names (TSgdGroups: tsgd_update, TAdamGroups: tadam_update)
// with the scalars of the entry's group.  EMA: the entry carries the EMA pointer, and the value just stored in p goes into the average
// from the register.  There an entry without a gradient (g null; wave-uniform) is EMA-only: no optimizer arithmetic, p is only read --
// the BatchNorm running statistics and parameters without .grad ride along in the same launch.
template <class E> __device__ __forceinline__ float topt_update(const E& e, const TSgdGroup& s, long idx) { return tsgd_update(e, s, idx); }
template <class E> __device__ __forceinline__ float topt_update(const E& e, const TAdamGroup& s, long idx) { return tadam_update(e, s, idx); }
template <bool EMA, class E, class GS>
__device__ __forceinline__ void topt_multi(const E* __restrict__ tab, int nt, const GS& gs, float d = 0.f, float omd = 0.f)
{
    tmulti_each(tab, nt, [&](const E& e, long idx) {
        const auto& s = gs.g[__builtin_amdgcn_readfirstlane(e.group) & (TOPT_MAX_GROUPS - 1)];
        if constexpr (EMA) {
            const float pn = e.g ? topt_update(e, s, idx) : e.p[idx];
            e.ema[idx] = tema_update(e.ema[idx], pn, d, omd);
        } else {
            topt_update(e, s, idx);
        }
    });
}
__global__ void __launch_bounds__(256) tsgd_group_kernel(const TOptEntry* __restrict__ tab, int nt, TSgdGroups gs) { topt_multi<false>(tab, nt, gs); }
__global__ void __launch_bounds__(256) tadam_group_kernel(const TOptEntry* __restrict__ tab, int nt, TAdamGroups gs) { topt_multi<false>(tab, nt, gs); }
__global__ void __launch_bounds__(256) tsgd_group_ema_kernel(const TOptEmaEntry* __restrict__ tab, int nt, TSgdGroups gs, float d, float omd)
{
    topt_multi<true>(tab, nt, gs, d, omd);
}
__global__ void __launch_bounds__(256) tadam_group_ema_kernel(const TOptEmaEntry* __restrict__ tab, int nt, TAdamGroups gs, float d, float omd)
{
    topt_multi<true>(tab, nt, gs, d, omd);
}

// the older entries: one tensor per launch (yf_train_adam_step; `e.n` elements from workgroup 0), and every tensor of one group
__global__ void __launch_bounds__(256) tadam_kernel(TAdamEntry e, TAdamGroup s)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < e.n) tadam_update(e, s, idx);
}
__global__ void __launch_bounds__(256) tadam_multi_kernel(const TAdamEntry* __restrict__ tab, int nt, TAdamGroup s)
{
    tmulti_each(tab, nt, [&](const TAdamEntry& e, long idx) { tadam_update(e, s, idx); });
}

// the average alone, any number of (src, ema, n) tensors in one launch (ModelEMA.update beside a torch.optim optimizer)
__global__ void __launch_bounds__(256) tema_multi_kernel(const TEmaEntry* __restrict__ tab, int nt, float d, float omd)
{
    tmulti_each(tab, nt, [&](const TEmaEntry& e, long idx) { e.ema[idx] = tema_update(e.ema[idx], e.src[idx], d, omd); });
}
