// yf_aug_kernels.hip -- the image half of the reference's DetectDataset.__getitem__ (src/model_training/dataloader/detect_dataset.py:90-103,
// :123-162) on the device, for a batch of same-size source frames in ONE launch:
//     img = cv2.cvtColor(ori_img, cv2.COLOR_BGR2GRAY)        (:96-97, 1-channel net on BGR frames)
//     img = cv2.resize(img, (input_shape[1], input_shape[0])) (:101-102)
//     img = cv2.GaussianBlur(img, (k, k), 0)                  (:135-141, k = 7 or 3 per frame; 5 is accepted as well)
//     img = np.fliplr(img)                                    (:142-143, per frame)
// -> u8 [N, H, W, C] and / or float32 [N, C, H, W] = (v - 128) / 255 (what DetectDataset.collate_fn's `(u8 - 128.0) / 255` gives once cast to
// float32, the same expression as the stem's fused u8 entry).  Channels keep cv2.imread's BGR order, as the reference's dataset does.
//   gray / resize: the arithmetic of yf_cv_kernels.hip (OpenCV's 8-bit BGR2GRAY with 14- or 15-bit coefficients; same size: a copy; exactly
//     1/2: the 2x2 mean (a + b + c + d + 2) >> 2; otherwise INTER_LINEAR through cv::resize's tables from launch_cv_tables).
//   blur: OpenCV's 8-bit fixed-point GaussianBlur for sigma = 0 (the ufixedpoint16 row pass and ufixedpoint32 column pass of
//     modules/imgproc/src/smooth.simd.hpp): taps in 1/256 units k3 = [64 128 64], k5 = [16 64 96 64 16], k7 = [8 28 56 72 56 28 8]; the row
//     pass is exact in uint16, dst = (sum_y k_y * row_y + 2^15) >> 16; BORDER_REFLECT_101 on all four sides; every channel on its own.
//   flip: after the blur (the taps and reflect-101 are symmetric, so the two commute; tests/test_gpu_dataset.py shows it).
// yf_augment_warp_u8 adds yolov5's geometric warp between the resize and the blur (warp_kernel, a second launch over the resized frames);
// yf_augment_mix_u8 adds yolov5's mixup of two resized, warped frames before the blur (mix_kernel, one launch; see below);
// yf_augment_mosaic_u8 yolov5's mosaic of four resized frames, warped and cropped back to the frame size (mosaic_kernel, one launch);
// yf_augment_letterbox_u8 is the ragged twin: frames of ANY sizes, letterboxed instead of squashed -- cv_letterbox_kernel (yf_cv_kernels.hip)
// into a scratch, then aug_kernel or warp_kernel over it: a fused single launch was measured and was not faster.
// One workgroup owns `tr` destination rows of one frame: it stages those rows plus a 3-row halo of the resized (gray) image in LDS (computed
// straight from the source bytes, as cv_pre_kernel does), runs the row pass into a uint16 LDS buffer and the column pass out of it.  A frame
// whose k is 0 stages no halo and skips both passes (k is uniform per workgroup).  Integer arithmetic only on the byte path.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/yolo_fastest_hip.h"
#include "yf_kernels.h"

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

constexpr int AUG_R = 3;                  // halo of the widest kernel (7 x 7)
constexpr int AUG_MAX_TR = 16;            // destination rows per workgroup at most
constexpr int AUG_LDS = 48 * 1024;        // LDS budget of one workgroup (tile + row-pass buffer)

// the taps, centred in 7 slots (a shorter kernel has zeros at the ends, which add nothing)
__constant__ int aug_taps[3][7] = {{0, 0, 64, 128, 64, 0, 0}, {0, 16, 64, 96, 64, 16, 0}, {8, 28, 56, 72, 56, 28, 8}};

struct AugArgs {
    const uint8_t* src;           // [n_src, sh, sw, sc]
    const int* index;             // [n] frame of the source stack per output frame, or null (frame n)
    int n_src, n, sh, sw, sc;
    int dh, dw, dc;
    int mode, gray;               // as CvArgs
    const int4* xtab;             // mode 2
    const int4* ytab;
    const int* params;            // [n] k (0, 3, 5, 7) | flip << 8, or null (no blur, no flip: launch 1 of yf_augment_warp_u8)
    uint8_t* u8;                  // [n, dh, dw, dc] or null
    float* x;                     // [n, dc, dh, dw] or null
    int tr, pitch;                // destination rows per workgroup; LDS row pitch of the u8 tile (bytes, multiple of 16)
};

// cv::borderInterpolate(p, n, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

template <int GRAY>   // 0: plain channel c; 14 / 15: BGR -> gray
__device__ __forceinline__ int src_px(const uint8_t* __restrict__ row, int x, int sc, int c)
{
    if constexpr (GRAY == 0) {
        return row[(long)x * sc + c];
    } else {
        const uint8_t* p = row + (long)x * 3;
        constexpr int RY = GRAY == 14 ? 4899 : 9798, GY = GRAY == 14 ? 9617 : 19235, BY = GRAY == 14 ? 1868 : 3735;
        return (p[0] * BY + p[1] * GY + p[2] * RY + (1 << (GRAY - 1))) >> GRAY;
    }
}

// The row pass (blurred frames only): sum_x k_x * tile, exact in uint16 (at most 255 * 256); tile [T][pitch] -> hb [T][dw * C].
template <int C>
__device__ __forceinline__ void blur_rows(const uint8_t* tile, uint16_t* hb, const int* taps, int k, int T, int dw, int pitch)
{
    const int re = dw * C;
    if (k) {
#pragma unroll 1
        for (int e = threadIdx.x; e < T * dw; e += 256) {
            const int r = e / dw, x = e - r * dw;
            const uint8_t* const tr = tile + r * pitch;
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 0;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const int xs = reflect101(x + i - AUG_R, dw);
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += taps[i] * tr[xs * C + c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) hb[r * re + x * C + c] = (uint16_t)acc[c];
        }
        __syncthreads();
    }
}

// The column pass + flips + stores of `rows` destination rows from dy0 on, 4 destination pixels per task.  fliplr mirrors the columns
// read, flipud the row written (dh - 1 - dy): both commute with the blur (symmetric taps, reflect-101).
template <int C>
__device__ __forceinline__ void blur_cols_store(const uint8_t* tile, const uint16_t* hb, const int* taps, int k, int n, int dy0, int rows,
                                                int dh, int dw, int pitch, bool flip, bool flipud, uint8_t* u8, float* xo)
{
    const int re = dw * C;
    const int quads = (dw + 3) >> 2;
#pragma unroll 1
    for (int t = threadIdx.x; t < rows * quads; t += 256) {
        const int r = t / quads, dx0 = (t - r * quads) * 4, dy = flipud ? dh - 1 - (dy0 + r) : dy0 + r;
        uint32_t packed[C];
        float fv[C][4];
#pragma unroll
        for (int w = 0; w < C; ++w) packed[w] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = dx0 + i;
            if (dx >= dw) break;
            const int sx = flip ? dw - 1 - dx : dx;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                int v;
                if (k) {
                    int acc = 0;
#pragma unroll
                    for (int j = 0; j < 7; ++j) acc += taps[j] * (int)hb[(r + j) * re + sx * C + c];
                    v = (acc + (1 << 15)) >> 16;
                } else {
                    v = tile[r * pitch + sx * C + c];
                }
                const int kk = i * C + c;
                packed[kk >> 2] |= (uint32_t)v << (8 * (kk & 3));
                fv[c][i] = ((float)v - 128.0f) / 255.0f;
            }
        }
        const int nb = dw - dx0 < 4 ? dw - dx0 : 4;
        if (u8) {
            uint8_t* o = u8 + (((long)n * dh + dy) * dw + dx0) * C;
            if (nb == 4 && ((reinterpret_cast<uintptr_t>(o) & 3) == 0)) {
#pragma unroll
                for (int w = 0; w < C; ++w) reinterpret_cast<uint32_t*>(o)[w] = packed[w];
            } else {
                for (int kk = 0; kk < nb * C; ++kk) o[kk] = (uint8_t)(packed[kk >> 2] >> (8 * (kk & 3)));
            }
        }
        if (xo) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float* o = xo + (((long)n * C + c) * dh + dy) * dw + dx0;
                if (nb == 4 && ((reinterpret_cast<uintptr_t>(o) & 15) == 0)) {
                    *reinterpret_cast<float4*>(o) = make_float4(fv[c][0], fv[c][1], fv[c][2], fv[c][3]);
                } else {
                    for (int i = 0; i < nb; ++i) o[i] = fv[c][i];
                }
            }
        }
    }
}

template <int GRAY, int MODE, int C>
__global__ void __launch_bounds__(256) aug_kernel(AugArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
    const int groups = (a.dh + a.tr - 1) / a.tr;
    const int n = blockIdx.x / groups, dy0 = (blockIdx.x - n * groups) * a.tr;
    const int f = a.index ? a.index[n] : n;
    if (f < 0 || f >= a.n_src) return;                       // an index outside the stack leaves its output frame untouched
    const int p = a.params ? a.params[n] : 0;                // no parameters: the resized frame as it is
    const int k = ((p & 15) == 3 || (p & 15) == 5 || (p & 15) == 7) ? (p & 15) : 0;
    const bool flip = (p >> 8) & 1;
    const int* const taps = k ? aug_taps[(k - 3) >> 1] : aug_taps[0];
    const int rows = min(a.tr, a.dh - dy0);
    const int halo = k ? AUG_R : 0;
    const int T = rows + 2 * halo;                            // staged rows: destination rows dy0 - halo .. dy0 + rows + halo - 1 (reflected)
    const uint8_t* const src = a.src + (long)f * a.sh * a.sw * a.sc;
    const long rs = (long)a.sw * a.sc;
    const int quads = (a.dw + 3) >> 2;
    uint8_t* const tile = aug_smem;                                                              // [T][pitch]
    uint16_t* const hb = reinterpret_cast<uint16_t*>(aug_smem + (size_t)(a.tr + 2 * AUG_R) * a.pitch);   // [T][dw * C]

    // ---- stage: cvtColor + resize of the tile's rows, 4 destination pixels (all channels) per task, one 4-byte LDS store per channel ----
#pragma unroll 1
    for (int t = threadIdx.x; t < T * quads; t += 256) {
        const int r = t / quads, dx0 = (t - r * quads) * 4;
        const int y = reflect101(dy0 - halo + r, a.dh);
        int y0 = y, y1 = y, b0 = 0, b1 = 0;
        if constexpr (MODE == 1) { y0 = 2 * y; y1 = 2 * y + 1; }
        if constexpr (MODE == 2) { const int4 ty = a.ytab[y]; y0 = ty.x; y1 = ty.y; b0 = ty.z; b1 = ty.w; }
        const uint8_t* const row0 = src + y0 * rs;
        const uint8_t* const row1 = src + y1 * rs;
        uint32_t packed[C];
#pragma unroll
        for (int w = 0; w < C; ++w) packed[w] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = dx0 + i;
            if (dx >= a.dw) break;
            int x0 = dx, x1 = dx, a0 = 0, a1 = 0;
            if constexpr (MODE == 1) { x0 = 2 * dx; x1 = 2 * dx + 1; }
            if constexpr (MODE == 2) { const int4 tx = a.xtab[dx]; x0 = tx.x; x1 = tx.y; a0 = tx.z; a1 = tx.w; }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                int v;
                if constexpr (MODE == 0) {
                    v = src_px<GRAY>(row0, x0, a.sc, c);
                } else if constexpr (MODE == 1) {
                    v = (src_px<GRAY>(row0, x0, a.sc, c) + src_px<GRAY>(row0, x1, a.sc, c) + src_px<GRAY>(row1, x0, a.sc, c) +
                         src_px<GRAY>(row1, x1, a.sc, c) + 2) >> 2;
                } else {
                    const int r0 = src_px<GRAY>(row0, x0, a.sc, c) * a0 + src_px<GRAY>(row0, x1, a.sc, c) * a1;
                    const int r1 = src_px<GRAY>(row1, x0, a.sc, c) * a0 + src_px<GRAY>(row1, x1, a.sc, c) * a1;
                    v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                }
                const int kk = i * C + c;
                packed[kk >> 2] |= (uint32_t)(v & 255) << (8 * (kk & 3));
            }
        }
        uint32_t* const o = reinterpret_cast<uint32_t*>(tile + r * a.pitch + dx0 * C);   // the pitch holds quads * 4 * C bytes
#pragma unroll
        for (int w = 0; w < C; ++w) o[w] = packed[w];
    }
    __syncthreads();

    blur_rows<C>(tile, hb, taps, k, T, a.dw, a.pitch);
    blur_cols_store<C>(tile, hb, taps, k, n, dy0, rows, a.dh, a.dw, a.pitch, flip, false, a.u8, a.x);
}

// ---- the geometric warp (yf_augment_warp_u8): launch 2, over the resized (gray) frames launch 1 left in the scratch ----
struct WarpArgs {
    const uint8_t* img;           // [n, dh, dw, C] the resized frames (aug_kernel without parameters)
    const int* index;             // as AugArgs: a frame whose index is outside the stack was not resized and is left untouched here too
    int n_src, n, dh, dw;
    const int* params;            // [n] k | fliplr << 8 | flipud << 9 | warp << 10 | perspective << 11
    const double* warp;           // [n, 8] output -> input coefficients (read for frames with bit 10)
    uint8_t* u8;
    float* x;
    int tr, pitch;
};
constexpr int WARP_FILL = 114;    // yolov5's border value, every channel

// Pillow's arithmetic (src/libImaging/Geometry.c: affine_transform / perspective_transform + bilinear_filter8) in IEEE double, one rounding
// per operation: no contraction into FMAs, and the correctly rounded division (no fast-math).  It stands once, in two halves that
// warp_sample (a frame in memory) and canvas_sample (the mosaic's virtual canvas) share.
// Half 1, coordinates and weights: the source position of destination pixel (x, y) in an sw x sh image -> false: fill (a NaN fills as
// well); otherwise the top-left tap (x0, y0), -1 .. sw - 1 and -1 .. sh - 1, and the two weights.
__device__ __forceinline__ bool warp_coords(int sh, int sw, const double (&m)[8], bool persp, int x, int y, int& x0, int& y0, double& ddx,
                                            double& ddy)
{
#pragma clang fp contract(off)
    const double xin = x + 0.5, yin = y + 0.5;
    double sx = (m[0] * xin + m[1] * yin) + m[2];
    double sy = (m[3] * xin + m[4] * yin) + m[5];
    if (persp) {
        const double den = (m[6] * xin + m[7] * yin) + 1.0;
        sx = sx / den;
        sy = sy / den;
    }
    if (!(sx >= 0.0 && sx < sw && sy >= 0.0 && sy < sh)) return false;    // a NaN fills as well
    sx -= 0.5;
    sy -= 0.5;
    const double fx = floor(sx), fy = floor(sy);
    ddx = sx - fx;
    ddy = sy - fy;
    x0 = (int)fx;
    y0 = (int)fy;
    return true;
}

// Half 2, the blend of one channel: v1 = warp_lerp on row y0, v2 the same on row y0 + 1 if that row exists, else v1; warp_finish.
__device__ __forceinline__ double warp_lerp(int a, int b, double ddx)
{
#pragma clang fp contract(off)
    return (double)a + (double)(b - a) * ddx;
}

__device__ __forceinline__ int warp_finish(double v1, double v2, double ddy)
{
#pragma clang fp contract(off)
    return (int)(v1 + (v2 - v1) * ddy);                                   // (uint8)v: a truncation; 0 <= v <= 255
}

// One bilinear sample of a frame in memory.  -> false: fill.
template <int C>
__device__ __forceinline__ bool warp_sample(const uint8_t* __restrict__ img, int dh, int dw, const double (&m)[8], bool persp, int x, int y,
                                            int (&v)[C])
{
    int x0, y0;
    double ddx, ddy;
    if (!warp_coords(dh, dw, m, persp, x, y, x0, y0, ddx, ddy)) return false;
    const int xa = max(x0, 0), xb = min(x0 + 1, dw - 1);
    const uint8_t* const r0 = img + ((long)max(y0, 0) * dw) * C;
    const bool below = y0 + 1 < dh;                                       // y0 + 1 >= 0 always
    const uint8_t* const r1 = img + ((long)(below ? y0 + 1 : 0) * dw) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int a0 = r0[xa * C + c], b0 = r0[xb * C + c];
        const double v1 = warp_lerp(a0, b0, ddx);
        double v2 = v1;
        if (below) {
            const int a1 = r1[xa * C + c], b1 = r1[xb * C + c];
            v2 = warp_lerp(a1, b1, ddx);
        }
        v[c] = warp_finish(v1, v2, ddy);
    }
    return true;
}

// One pixel of a resized frame as the blur sees it: the bilinear sample under the frame's coefficients (114 outside), or the frame's own
// byte for a frame without the warp bit.
template <int C>
__device__ __forceinline__ void frame_px(const uint8_t* __restrict__ img, int dh, int dw, bool warped, const double (&m)[8], bool persp, int x,
                                         int y, int (&v)[C])
{
    if (!warped) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = img[((long)y * dw + x) * C + c];
    } else if (!warp_sample<C>(img, dh, dw, m, persp, x, y, v)) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = WARP_FILL;
    }
}

// Built like aug_kernel: one workgroup owns `tr` destination rows of one frame and stages them plus the blur halo (reflect-101 on the
// WARPED image) in LDS, each staged pixel a bilinear sample of the resized frame (or that frame's own pixel without bit 10: then the
// bytes are yf_augment_u8's); the blur passes are aug_kernel's; both flips at the store.
template <int C>
__global__ void __launch_bounds__(256) warp_kernel(WarpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
    const int groups = (a.dh + a.tr - 1) / a.tr;
    const int n = blockIdx.x / groups, dy0 = (blockIdx.x - n * groups) * a.tr;
    const int f = a.index ? a.index[n] : n;
    if (f < 0 || f >= a.n_src) return;
    const int p = a.params[n];
    const int k = ((p & 15) == 3 || (p & 15) == 5 || (p & 15) == 7) ? (p & 15) : 0;
    const bool fliplr = (p >> 8) & 1, flipud = (p >> 9) & 1, warped = (p >> 10) & 1, persp = (p >> 11) & 1;
    const int* const taps = k ? aug_taps[(k - 3) >> 1] : aug_taps[0];
    const int rows = min(a.tr, a.dh - dy0);
    const int halo = k ? AUG_R : 0;
    const int T = rows + 2 * halo;
    const uint8_t* const img = a.img + (long)n * a.dh * a.dw * C;
    const int quads = (a.dw + 3) >> 2;
    uint8_t* const tile = aug_smem;                                                              // [T][pitch]
    uint16_t* const hb = reinterpret_cast<uint16_t*>(aug_smem + (size_t)(a.tr + 2 * AUG_R) * a.pitch);   // [T][dw * C]
    double m[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (warped) {
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = a.warp[(long)n * 8 + i];
    }

    // ---- stage: 4 destination pixels (all channels) per task, one 4-byte LDS store per channel ----
#pragma unroll 1
    for (int t = threadIdx.x; t < T * quads; t += 256) {
        const int r = t / quads, dx0 = (t - r * quads) * 4;
        const int y = reflect101(dy0 - halo + r, a.dh);
        uint32_t packed[C];
#pragma unroll
        for (int w = 0; w < C; ++w) packed[w] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = dx0 + i;
            if (dx >= a.dw) break;
            int v[C];
            frame_px<C>(img, a.dh, a.dw, warped, m, persp, dx, y, v);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int kk = i * C + c;
                packed[kk >> 2] |= (uint32_t)(v[c] & 255) << (8 * (kk & 3));
            }
        }
        uint32_t* const o = reinterpret_cast<uint32_t*>(tile + r * a.pitch + dx0 * C);
#pragma unroll
        for (int w = 0; w < C; ++w) o[w] = packed[w];
    }
    __syncthreads();

    blur_rows<C>(tile, hb, taps, k, T, a.dw, a.pitch);
    blur_cols_store<C>(tile, hb, taps, k, n, dy0, rows, a.dh, a.dw, a.pitch, fliplr, flipud, a.u8, a.x);
}

// ---- mixup (yf_augment_mix_u8): one launch over frames that are already resized (and gray) ----
struct MixArgs {
    const uint8_t* frames;        // [n_frames, dh, dw, C] resized frames (aug_kernel without parameters)
    int n_frames, n, dh, dw;
    const int* first;             // [n] frame the output is made of; outside 0 .. n_frames - 1: the output frame is left untouched
    const int* second;            // [n] the partner: negative = none; >= n_frames: the output frame is left untouched
    const int* params;            // [n] WarpArgs' bits (the first frame and the mixture) | partner warped << 12 | partner perspective << 13
    const double* warp;           // [n, 2, 8] coefficients of the first frame and of the partner (each read with its warp bit)
    const double* ratio;          // [n] r: mix = trunc(first * r + partner * (1 - r)) (read for frames with a partner)
    uint8_t* u8;
    float* x;
    int tr, pitch;
};

// yolov5's `(im * r + im2 * (1 - r)).astype(np.uint8)` for one byte pair: IEEE double, one rounding per operation (no FMA, no
// rearrangement: with r = 0.4809054919537687, 127 mixed with 127 is 126).  q = 1.0 - r.  The clamp changes nothing for 0 <= r <= 1; it
// keeps a caller's bad ratio or a NaN (-> 0) from wrapping in the conversion.
__device__ __forceinline__ int mix_px(int a, int b, double r, double q)
{
#pragma clang fp contract(off)
    const double t = (double)a * r + (double)b * q;
    return t >= 0.0 ? (t <= 255.0 ? (int)t : 255) : 0;
}

// The staging of mix_kernel: 4 destination pixels (all channels) per task, each the first frame's pixel (frame_px) and, with PARTNER,
// that blended with the partner's pixel under the partner's own coefficients.
template <int C, bool PARTNER>
__device__ __forceinline__ void mix_stage(const MixArgs& a, uint8_t* tile, const uint8_t* __restrict__ img, const uint8_t* __restrict__ img2,
                                          int dy0, int halo, int T, bool warped, bool persp, const double (&m)[8], bool warped2, bool persp2,
                                          const double (&m2)[8], double r, double q)
{
    const int quads = (a.dw + 3) >> 2;
#pragma unroll 1
    for (int t = threadIdx.x; t < T * quads; t += 256) {
        const int row = t / quads, dx0 = (t - row * quads) * 4;
        const int y = reflect101(dy0 - halo + row, a.dh);
        uint32_t packed[C];
#pragma unroll
        for (int w = 0; w < C; ++w) packed[w] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = dx0 + i;
            if (dx >= a.dw) break;
            int v[C];
            frame_px<C>(img, a.dh, a.dw, warped, m, persp, dx, y, v);
            if constexpr (PARTNER) {
                int u[C];
                frame_px<C>(img2, a.dh, a.dw, warped2, m2, persp2, dx, y, u);
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = mix_px(v[c], u[c], r, q);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int kk = i * C + c;
                packed[kk >> 2] |= (uint32_t)(v[c] & 255) << (8 * (kk & 3));
            }
        }
        uint32_t* const o = reinterpret_cast<uint32_t*>(tile + row * a.pitch + dx0 * C);
#pragma unroll
        for (int w = 0; w < C; ++w) o[w] = packed[w];
    }
}

// Built like warp_kernel: one workgroup owns `tr` destination rows of one output frame and stages them plus the blur halo (reflect-101 on
// the MIXTURE) in LDS; a frame without a partner is staged exactly as warp_kernel stages it (no blend); the blur passes and both flips
// are the shared ones.  k, the flags, "has partner", r, 1 - r and the sixteen coefficients are uniform per workgroup.
template <int C>
__global__ void __launch_bounds__(256) mix_kernel(MixArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
    const int groups = (a.dh + a.tr - 1) / a.tr;
    const int n = blockIdx.x / groups, dy0 = (blockIdx.x - n * groups) * a.tr;
    const int f = a.first[n], f2 = a.second[n];
    if (f < 0 || f >= a.n_frames || f2 >= a.n_frames) return;  // nothing is read out of bounds; the output frame stays as it was
    const bool partner = f2 >= 0;
    const int p = a.params[n];
    const int k = ((p & 15) == 3 || (p & 15) == 5 || (p & 15) == 7) ? (p & 15) : 0;
    const bool fliplr = (p >> 8) & 1, flipud = (p >> 9) & 1, warped = (p >> 10) & 1, persp = (p >> 11) & 1;
    const bool warped2 = partner && ((p >> 12) & 1), persp2 = (p >> 13) & 1;
    const int* const taps = k ? aug_taps[(k - 3) >> 1] : aug_taps[0];
    const int rows = min(a.tr, a.dh - dy0);
    const int halo = k ? AUG_R : 0;
    const int T = rows + 2 * halo;
    const long frame = (long)a.dh * a.dw * C;
    const uint8_t* const img = a.frames + f * frame;
    uint8_t* const tile = aug_smem;                                                              // [T][pitch]
    uint16_t* const hb = reinterpret_cast<uint16_t*>(aug_smem + (size_t)(a.tr + 2 * AUG_R) * a.pitch);   // [T][dw * C]
    double m[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, m2[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (warped) {
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = a.warp[(long)n * 16 + i];
    }
    if (warped2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) m2[i] = a.warp[(long)n * 16 + 8 + i];
    }

    if (partner) {
#pragma clang fp contract(off)
        const double r = a.ratio[n], q = 1.0 - r;
        mix_stage<C, true>(a, tile, img, a.frames + f2 * frame, dy0, halo, T, warped, persp, m, warped2, persp2, m2, r, q);
    } else {
        mix_stage<C, false>(a, tile, img, img, dy0, halo, T, warped, persp, m, false, false, m2, 0.0, 0.0);
    }
    __syncthreads();

    blur_rows<C>(tile, hb, taps, k, T, a.dw, a.pitch);
    blur_cols_store<C>(tile, hb, taps, k, n, dy0, rows, a.dh, a.dw, a.pitch, fliplr, flipud, a.u8, a.x);
}

// ---- mosaic (yf_augment_mosaic_u8): one launch over frames that are already resized (and gray) ----
struct MosaicArgs {
    const uint8_t* frames;        // [n_frames, dh, dw, C] resized frames (aug_kernel without parameters): the tiles, all dh x dw
    int n_frames, n, dh, dw;
    const int* tiles;             // [n, 4] top-left, top-right, bottom-left, bottom-right; [n][1] < 0: no mosaic, frame [n][0] as warp_kernel
    const int* centre;            // [n, 2] (xc, yc) on the 2 dw x 2 dh canvas (read for mosaics)
    const int* params;            // [n] WarpArgs' bits; a mosaic always samples through its coefficients (bit 10 is not consulted)
    const double* warp;           // [n, 8]
    uint8_t* u8;
    float* x;
    int tr, pitch;
};

// yolov5's load_mosaic canvas, never in memory: four dh x dw tiles around (xc, yc) on a 2 dw x 2 dh canvas of 114s.  Per quadrant the
// canvas rectangle [x1a, x2a) x [y1a, y2a) and the pads (canvas = tile + pad) by load_mosaic's formulas: x1a / x2a and padw = x1a - x1b
// depend on the column half only (left of xc or not), y1a / y2a and padh = y1a - y1b on the row half only, so six values per axis hold all four.
struct Canvas {
    const uint8_t* tl; const uint8_t* tr; const uint8_t* bl; const uint8_t* br;   // the four tiles
    int xc, yc, dw;
    int lx1, lx2, lpad, rx1, rx2, rpad;                                            // left and right column half: x1a, x2a, padw
    int ty1, ty2, tpad, by1, by2, bpad;                                            // top and bottom row half: y1a, y2a, padh
};

__device__ __forceinline__ void canvas_of(Canvas& cv, int xc, int yc, int dh, int dw)
{
    cv.xc = xc; cv.yc = yc; cv.dw = dw;
    cv.lx1 = max(xc - dw, 0); cv.lx2 = xc;                   cv.lpad = cv.lx1 - (dw - (cv.lx2 - cv.lx1));   // x1b = w - (x2a - x1a)
    cv.rx1 = xc;              cv.rx2 = min(xc + dw, 2 * dw); cv.rpad = cv.rx1;                              // x1b = 0
    cv.ty1 = max(yc - dh, 0); cv.ty2 = yc;                   cv.tpad = cv.ty1 - (dh - (cv.ty2 - cv.ty1));
    cv.by1 = yc;              cv.by2 = min(yc + dh, 2 * dh); cv.bpad = cv.by1;
}

// One canvas pixel (cx, cy), 0 <= cx < 2 dw, 0 <= cy < 2 dh: the quadrant from cx < xc, cy < yc; that quadrant's tile byte at (cx - padw,
// cy - padh) if (cx, cy) lies inside the tile's canvas rectangle, else 114.  Inside the rectangle the tile coordinates lie inside the tile
// (the source rectangle is the rectangle minus the pads), so nothing is read out of bounds.  Every field is read first and
// the selects act on the values: the struct stays in registers (a select between fields becomes an indexed load from scratch memory).
template <int C>
__device__ __forceinline__ void canvas_px(const Canvas& cv, int cx, int cy, int (&v)[C])
{
    const uint8_t* const tl = cv.tl; const uint8_t* const tr = cv.tr; const uint8_t* const bl = cv.bl; const uint8_t* const br = cv.br;
    const int lx1 = cv.lx1, lx2 = cv.lx2, lpad = cv.lpad, rx1 = cv.rx1, rx2 = cv.rx2, rpad = cv.rpad;
    const int ty1 = cv.ty1, ty2 = cv.ty2, tpad = cv.tpad, by1 = cv.by1, by2 = cv.by2, bpad = cv.bpad;
    const bool left = cx < cv.xc, top = cy < cv.yc;
    const int x1 = left ? lx1 : rx1, x2 = left ? lx2 : rx2, padw = left ? lpad : rpad;
    const int y1 = top ? ty1 : by1, y2 = top ? ty2 : by2, padh = top ? tpad : bpad;
    if (cx >= x1 && cx < x2 && cy >= y1 && cy < y2) {
        const uint8_t* const t = top ? (left ? tl : tr) : (left ? bl : br);
        const uint8_t* const p = t + ((long)(cy - padh) * cv.dw + (cx - padw)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = p[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = WARP_FILL;
    }
}

// warp_sample over the virtual canvas: inside test against 2 dw x 2 dh, taps clamped to the canvas, each fetched through canvas_px, so a
// footprint on a seam mixes two to four tiles, or a tile and 114, as on the materialised canvas.  -> false: fill.
template <int C>
__device__ __forceinline__ bool canvas_sample(const Canvas& cv, int dh, int dw, const double (&m)[8], bool persp, int x, int y, int (&v)[C])
{
    int x0, y0;
    double ddx, ddy;
    if (!warp_coords(2 * dh, 2 * dw, m, persp, x, y, x0, y0, ddx, ddy)) return false;
    const int xa = max(x0, 0), xb = min(x0 + 1, 2 * dw - 1), ya = max(y0, 0);
    const bool below = y0 + 1 < 2 * dh;
    int a0[C], b0[C], a1[C], b1[C];
    canvas_px<C>(cv, xa, ya, a0);
    canvas_px<C>(cv, xb, ya, b0);
    if (below) {
        canvas_px<C>(cv, xa, y0 + 1, a1);
        canvas_px<C>(cv, xb, y0 + 1, b1);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double v1 = warp_lerp(a0[c], b0[c], ddx);
        double v2 = v1;
        if (below) v2 = warp_lerp(a1[c], b1[c], ddx);
        v[c] = warp_finish(v1, v2, ddy);
    }
    return true;
}

// Built like warp_kernel / mix_kernel: one workgroup owns `tr` destination rows of one output frame and stages them plus the blur halo
// (reflect-101 on the WARPED image) in LDS; a staged pixel of a mosaic is canvas_sample's, of any other frame frame_px's (warp_kernel's
// bytes); the blur passes and both flips are the shared ones.  Mosaic or not, the tiles, the centre, the rectangles, k, the flags and the
// coefficients are uniform per workgroup.
template <int C>
__global__ void __launch_bounds__(256) mosaic_kernel(MosaicArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
    const int groups = (a.dh + a.tr - 1) / a.tr;
    const int n = blockIdx.x / groups, dy0 = (blockIdx.x - n * groups) * a.tr;
    const int f = a.tiles[(long)n * 4], f1 = a.tiles[(long)n * 4 + 1];
    if (f < 0 || f >= a.n_frames) return;                     // nothing is read out of bounds; the output frame stays as it was
    const bool mosaic = f1 >= 0;
    const long frame = (long)a.dh * a.dw * C;
    const uint8_t* const img = a.frames + f * frame;          // the frame itself, or the top-left tile
    // The canvas record is read for a mosaic only.  It is filled on both paths all the same (centre (0, 0), every tile the frame): filling
    // it under `if (mosaic)` alone compiles to 4 / 19 spilled SGPRs (1 / 3 channels) where this form has 2 / 7.
    Canvas cv;
    cv.tl = cv.tr = cv.bl = cv.br = img;
    int xc = 0, yc = 0;
    if (mosaic) {
        const int f2 = a.tiles[(long)n * 4 + 2], f3 = a.tiles[(long)n * 4 + 3];
        if (f1 >= a.n_frames || f2 < 0 || f2 >= a.n_frames || f3 < 0 || f3 >= a.n_frames) return;
        xc = a.centre[(long)n * 2];
        yc = a.centre[(long)n * 2 + 1];
        if (xc < 0 || xc > 2 * a.dw || yc < 0 || yc > 2 * a.dh) return;
        cv.tr = a.frames + f1 * frame; cv.bl = a.frames + f2 * frame; cv.br = a.frames + f3 * frame;
    }
    canvas_of(cv, xc, yc, a.dh, a.dw);
    const int p = a.params[n];
    const int k = ((p & 15) == 3 || (p & 15) == 5 || (p & 15) == 7) ? (p & 15) : 0;
    const bool fliplr = (p >> 8) & 1, flipud = (p >> 9) & 1, warped = mosaic || ((p >> 10) & 1), persp = (p >> 11) & 1;
    const int* const taps = k ? aug_taps[(k - 3) >> 1] : aug_taps[0];
    const int rows = min(a.tr, a.dh - dy0);
    const int halo = k ? AUG_R : 0;
    const int T = rows + 2 * halo;
    const int quads = (a.dw + 3) >> 2;
    uint8_t* const tile = aug_smem;                                                              // [T][pitch]
    uint16_t* const hb = reinterpret_cast<uint16_t*>(aug_smem + (size_t)(a.tr + 2 * AUG_R) * a.pitch);   // [T][dw * C]
    double m[8] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (warped) {
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = a.warp[(long)n * 8 + i];
    }

    // ---- stage: 4 destination pixels (all channels) per task, one 4-byte LDS store per channel ----
#pragma unroll 1
    for (int t = threadIdx.x; t < T * quads; t += 256) {
        const int r = t / quads, dx0 = (t - r * quads) * 4;
        const int y = reflect101(dy0 - halo + r, a.dh);
        uint32_t packed[C];
#pragma unroll
        for (int w = 0; w < C; ++w) packed[w] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dx = dx0 + i;
            if (dx >= a.dw) break;
            int v[C];
            if (!mosaic) {
                frame_px<C>(img, a.dh, a.dw, warped, m, persp, dx, y, v);
            } else if (!canvas_sample<C>(cv, a.dh, a.dw, m, persp, dx, y, v)) {
#pragma unroll
                for (int c = 0; c < C; ++c) v[c] = WARP_FILL;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int kk = i * C + c;
                packed[kk >> 2] |= (uint32_t)(v[c] & 255) << (8 * (kk & 3));
            }
        }
        uint32_t* const o = reinterpret_cast<uint32_t*>(tile + r * a.pitch + dx0 * C);
#pragma unroll
        for (int w = 0; w < C; ++w) o[w] = packed[w];
    }
    __syncthreads();

    blur_rows<C>(tile, hb, taps, k, T, a.dw, a.pitch);
    blur_cols_store<C>(tile, hb, taps, k, n, dy0, rows, a.dh, a.dw, a.pitch, fliplr, flipud, a.u8, a.x);
}

template <int GRAY, int C>
void launch_aug_mode(const AugArgs& a, size_t lds, hipStream_t s)
{
    const unsigned grid = (unsigned)((long)a.n * ((a.dh + a.tr - 1) / a.tr));
    if (a.mode == 0) hipLaunchKernelGGL((aug_kernel<GRAY, 0, C>), dim3(grid), dim3(256), lds, s, a);
    else if (a.mode == 1) hipLaunchKernelGGL((aug_kernel<GRAY, 1, C>), dim3(grid), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((aug_kernel<GRAY, 2, C>), dim3(grid), dim3(256), lds, s, a);
}

// The LDS geometry aug_kernel, warp_kernel, mix_kernel and mosaic_kernel share: destination rows per workgroup, the u8 tile's row pitch and the LDS bytes of
// a workgroup for N frames of dst_h x dst_w x dst_c.
int aug_tile(const char* who, int N, int dst_h, int dst_w, int dst_c, int& tr_out, int& pitch, size_t& lds)
{
    const int quads = (dst_w + 3) >> 2;
    pitch = (quads * 4 * dst_c + 15) & ~15;
    const long per_row = (long)pitch + 2L * dst_w * dst_c;   // u8 tile row + uint16 row-pass row
    const long tr = AUG_LDS / per_row - 2 * AUG_R;
    if (tr < 1) return fail(YF_E_INVALID, "%s: rows of %d x %d bytes do not fit the LDS tile", who, dst_w, dst_c);
    tr_out = tr < AUG_MAX_TR ? (int)tr : AUG_MAX_TR;
    lds = (size_t)(tr_out + 2 * AUG_R) * per_row;
    const long groups = (long)N * ((dst_h + tr_out - 1) / tr_out);
    if (groups > 0x7fffffffL) return fail(YF_E_INVALID, "%s: batch too large for one launch", who);
    return YF_OK;
}

// The arguments yf_augment_u8 and yf_augment_warp_u8 share, checked, into AugArgs (parameters left to the caller) + the LDS bytes of a
// workgroup; `who` names the entry in the messages.
int aug_setup(const char* who, const uint8_t* d_src, int src_h, int src_w, int src_c, const int* d_index, int n_src, int N, const void* d_xtab,
              const void* d_ytab, int dst_h, int dst_w, int dst_c, int gray_bits, uint8_t* d_u8, float* d_x, AugArgs& a, size_t& lds)
{
    if (!d_src || (!d_u8 && !d_x) || N <= 0 || n_src <= 0 || (!d_index && n_src < N))
        return fail(YF_E_INVALID, "%s: null pointer, no output, N <= 0 or fewer source frames than N without an index table", who);
    if (src_h <= 0 || src_w <= 0 || src_h > 16384 || src_w > 16384 || dst_h <= 0 || dst_w <= 0 || dst_h > 16384 || dst_w > 16384)
        return fail(YF_E_INVALID, "%s: source %dx%d / destination %dx%d", who, src_h, src_w, dst_h, dst_w);
    a.src = d_src; a.index = d_index; a.n_src = n_src; a.n = N; a.sh = src_h; a.sw = src_w; a.sc = src_c; a.dh = dst_h; a.dw = dst_w; a.dc = dst_c;
    a.u8 = d_u8; a.x = d_x;
    if (src_c == 3 && dst_c == 1) {
        if (gray_bits != 0 && gray_bits != 14 && gray_bits != 15) return fail(YF_E_INVALID, "gray_bits must be 14, 15 or 0 (= 15)");
        a.gray = gray_bits == 14 ? 14 : 15;
    } else if (src_c == dst_c && (src_c == 1 || src_c == 3)) {
        a.gray = 0;
    } else {
        return fail(YF_E_INVALID, "%s: %d-channel frames from %d-channel sources (gray from BGR, or 1 / 3 channels as they are)", who, dst_c, src_c);
    }
    a.mode = (src_h == dst_h && src_w == dst_w) ? 0 : (src_h == 2 * dst_h && src_w == 2 * dst_w) ? 1 : 2;
    if (a.mode == 2) {
        if (!d_xtab || !d_ytab) return fail(YF_E_INVALID, "%s: a %dx%d -> %dx%d resize needs the tables of yf_cv_resize_tables", who, src_h, src_w, dst_h, dst_w);
        a.xtab = static_cast<const int4*>(d_xtab); a.ytab = static_cast<const int4*>(d_ytab);
    }
    return aug_tile(who, N, dst_h, dst_w, dst_c, a.tr, a.pitch, lds);
}

void launch_aug(const AugArgs& a, size_t lds, hipStream_t s)
{
    if (a.gray == 14) launch_aug_mode<14, 1>(a, lds, s);
    else if (a.gray == 15) launch_aug_mode<15, 1>(a, lds, s);
    else if (a.dc == 1) launch_aug_mode<0, 1>(a, lds, s);
    else launch_aug_mode<0, 3>(a, lds, s);
}

}  // namespace

extern "C" {

int yf_cv_resize_tables(int device, int src_h, int src_w, int dst_h, int dst_w, void* d_xtab, void* d_ytab, void* stream)
{
    if (src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || src_h > 16384 || src_w > 16384 || dst_h > 16384 || dst_w > 16384 || !d_xtab || !d_ytab)
        return fail(YF_E_INVALID, "yf_cv_resize_tables: bad argument");
    HIP_OK(hipSetDevice(device));
    yf::launch_cv_tables(src_h, src_w, dst_h, dst_w, static_cast<int4*>(d_xtab), static_cast<int4*>(d_ytab), (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_augment_u8(int device, const uint8_t* d_src, int src_h, int src_w, int src_c, const int* d_index, int n_src, int N, const void* d_xtab,
                  const void* d_ytab, int dst_h, int dst_w, int dst_c, int gray_bits, const int* d_params, uint8_t* d_u8, float* d_x, void* stream)
{
    AugArgs a{};
    size_t lds;
    if (!d_params) return fail(YF_E_INVALID, "yf_augment_u8: null d_params");
    const int rc = aug_setup("yf_augment_u8", d_src, src_h, src_w, src_c, d_index, n_src, N, d_xtab, d_ytab, dst_h, dst_w, dst_c, gray_bits, d_u8, d_x,
                             a, lds);
    if (rc != YF_OK) return rc;
    a.params = d_params;
    HIP_OK(hipSetDevice(device));
    launch_aug(a, lds, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_augment_warp_u8(int device, const uint8_t* d_src, int src_h, int src_w, int src_c, const int* d_index, int n_src, int N, const void* d_xtab,
                       const void* d_ytab, int dst_h, int dst_w, int dst_c, int gray_bits, const int* d_params, const double* d_warp,
                       uint8_t* d_scratch, uint8_t* d_u8, float* d_x, void* stream)
{
    AugArgs a{};
    size_t lds;
    if (!d_params || !d_warp || !d_scratch) return fail(YF_E_INVALID, "yf_augment_warp_u8: null d_params, d_warp or d_scratch");
    const int rc = aug_setup("yf_augment_warp_u8", d_src, src_h, src_w, src_c, d_index, n_src, N, d_xtab, d_ytab, dst_h, dst_w, dst_c, gray_bits,
                             d_u8, d_x, a, lds);
    if (rc != YF_OK) return rc;
    WarpArgs w{};
    w.img = d_scratch; w.index = d_index; w.n_src = n_src; w.n = N; w.dh = dst_h; w.dw = dst_w; w.params = d_params; w.warp = d_warp;
    w.u8 = d_u8; w.x = d_x; w.tr = a.tr; w.pitch = a.pitch;
    a.params = nullptr; a.u8 = d_scratch; a.x = nullptr;      // launch 1: gray + resize alone, into the scratch
    HIP_OK(hipSetDevice(device));
    const hipStream_t s = (hipStream_t)stream;
    launch_aug(a, lds, s);
    HIP_OK(hipGetLastError());
    const unsigned grid = (unsigned)((long)N * ((dst_h + a.tr - 1) / a.tr));
    if (dst_c == 1) hipLaunchKernelGGL((warp_kernel<1>), dim3(grid), dim3(256), lds, s, w);
    else hipLaunchKernelGGL((warp_kernel<3>), dim3(grid), dim3(256), lds, s, w);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_augment_letterbox_u8(int device, int N, const void* const* d_frames, const int* heights, const int* widths, int gray_bits, int dst_h,
                            int dst_w, const int* d_params, int geometric, const double* d_warp, uint8_t* d_scratch, uint8_t* d_u8, float* d_x,
                            void* d_table, size_t table_bytes, void* h_table_pinned, void* stream)
{
    const char* who = "yf_augment_letterbox_u8";
    if (!d_u8 && !d_x) return fail(YF_E_INVALID, "%s: no output", who);
    if (!d_params || !d_scratch) return fail(YF_E_INVALID, "%s: null d_params or d_scratch", who);
    if (geometric && !d_warp) return fail(YF_E_INVALID, "%s: a frame with bit 9 or 10 needs d_warp", who);
    if (gray_bits != 0 && gray_bits != 14 && gray_bits != 15) return fail(YF_E_INVALID, "%s: gray_bits must be 0 (three channels), 14 or 15", who);
    if (N <= 0 || dst_h <= 0 || dst_w <= 0 || dst_h > YF_LB_MAX_SIDE || dst_w > YF_LB_MAX_SIDE)
        return fail(YF_E_INVALID, "%s: N %d, destination %dx%d", who, N, dst_h, dst_w);
    const int C = gray_bits ? 1 : 3;
    AugArgs a{};
    size_t lds;
    if (int rc = aug_tile(who, N, dst_h, dst_w, C, a.tr, a.pitch, lds)) return rc;
    if ((long)N * ((dst_h + yf::LB_TR - 1) / yf::LB_TR) > 0x7fffffffL)         // launch 1's grid: refused here, before the table is written
        return fail(YF_E_INVALID, "%s: %d frames of %d rows are more workgroups than one launch takes", who, N, dst_h);
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = yf::lb_upload_table(who, device, N, d_frames, heights, widths, gray_bits, dst_h, dst_w, d_table, table_bytes, h_table_pinned, s))
        return rc;
    // launch 1: the letterboxed (gray) frames, into the scratch
    if (yf::launch_cv_letterbox(static_cast<const yf::LbEntry*>(d_table), N, gray_bits, dst_h, dst_w, d_scratch, s))
        return fail(YF_E_INVALID, "%s: %d frames of %d rows are more workgroups than one launch takes", who, N, dst_h);
    HIP_OK(hipGetLastError());
    // launch 2 over the scratch as N same-size sources: yf_augment_u8's kernel, or with a warped / flipud frame yf_augment_warp_u8's second
    if (!geometric) {
        a.src = d_scratch; a.index = nullptr; a.n_src = N; a.n = N; a.sh = dst_h; a.sw = dst_w; a.sc = C; a.dh = dst_h; a.dw = dst_w; a.dc = C;
        a.mode = 0; a.gray = 0; a.params = d_params; a.u8 = d_u8; a.x = d_x;
        launch_aug(a, lds, s);
    } else {
        WarpArgs w{};
        w.img = d_scratch; w.index = nullptr; w.n_src = N; w.n = N; w.dh = dst_h; w.dw = dst_w; w.params = d_params; w.warp = d_warp;
        w.u8 = d_u8; w.x = d_x; w.tr = a.tr; w.pitch = a.pitch;
        const unsigned grid = (unsigned)((long)N * ((dst_h + a.tr - 1) / a.tr));
        if (C == 1) hipLaunchKernelGGL((warp_kernel<1>), dim3(grid), dim3(256), lds, s, w);
        else hipLaunchKernelGGL((warp_kernel<3>), dim3(grid), dim3(256), lds, s, w);
    }
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_augment_mix_u8(int device, const uint8_t* d_frames, int n_frames, int N, int h, int w, int c, const int* d_first, const int* d_second,
                      const int* d_params, const double* d_warp, const double* d_ratio, uint8_t* d_u8, float* d_x, void* stream)
{
    if (!d_frames || !d_first || !d_second || !d_params || !d_warp || !d_ratio || (!d_u8 && !d_x) || N <= 0 || n_frames <= 0)
        return fail(YF_E_INVALID, "yf_augment_mix_u8: null pointer, no output, N <= 0 or n_frames <= 0");
    if (h <= 0 || w <= 0 || h > 16384 || w > 16384) return fail(YF_E_INVALID, "yf_augment_mix_u8: frames of %dx%d", h, w);
    if (c != 1 && c != 3) return fail(YF_E_INVALID, "yf_augment_mix_u8: %d-channel frames (1 or 3)", c);
    MixArgs m{};
    size_t lds;
    const int rc = aug_tile("yf_augment_mix_u8", N, h, w, c, m.tr, m.pitch, lds);
    if (rc != YF_OK) return rc;
    m.frames = d_frames; m.n_frames = n_frames; m.n = N; m.dh = h; m.dw = w; m.first = d_first; m.second = d_second; m.params = d_params;
    m.warp = d_warp; m.ratio = d_ratio; m.u8 = d_u8; m.x = d_x;
    HIP_OK(hipSetDevice(device));
    const unsigned grid = (unsigned)((long)N * ((h + m.tr - 1) / m.tr));
    if (c == 1) hipLaunchKernelGGL((mix_kernel<1>), dim3(grid), dim3(256), lds, (hipStream_t)stream, m);
    else hipLaunchKernelGGL((mix_kernel<3>), dim3(grid), dim3(256), lds, (hipStream_t)stream, m);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_augment_mosaic_u8(int device, const uint8_t* d_frames, int n_frames, int N, int h, int w, int c, const int* d_tiles, const int* d_centre,
                         const int* d_params, const double* d_warp, uint8_t* d_u8, float* d_x, void* stream)
{
    if (!d_frames || !d_tiles || !d_centre || !d_params || !d_warp || (!d_u8 && !d_x) || N <= 0 || n_frames <= 0)
        return fail(YF_E_INVALID, "yf_augment_mosaic_u8: null pointer, no output, N <= 0 or n_frames <= 0");
    if (h <= 0 || w <= 0 || h > 16384 || w > 16384) return fail(YF_E_INVALID, "yf_augment_mosaic_u8: frames of %dx%d", h, w);
    if (c != 1 && c != 3) return fail(YF_E_INVALID, "yf_augment_mosaic_u8: %d-channel frames (1 or 3)", c);
    MosaicArgs m{};
    size_t lds;
    const int rc = aug_tile("yf_augment_mosaic_u8", N, h, w, c, m.tr, m.pitch, lds);
    if (rc != YF_OK) return rc;
    m.frames = d_frames; m.n_frames = n_frames; m.n = N; m.dh = h; m.dw = w; m.tiles = d_tiles; m.centre = d_centre; m.params = d_params;
    m.warp = d_warp; m.u8 = d_u8; m.x = d_x;
    HIP_OK(hipSetDevice(device));
    const unsigned grid = (unsigned)((long)N * ((h + m.tr - 1) / m.tr));
    if (c == 1) hipLaunchKernelGGL((mosaic_kernel<1>), dim3(grid), dim3(256), lds, (hipStream_t)stream, m);
    else hipLaunchKernelGGL((mosaic_kernel<3>), dim3(grid), dim3(256), lds, (hipStream_t)stream, m);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

}  // extern "C"
