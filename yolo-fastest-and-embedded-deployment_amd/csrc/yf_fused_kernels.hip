// yf_fused_kernels.hip -- block-fused kernels: the wide (expanded) tensors of the net never leave the CU.
//
// fused_block_kernel:  pw-expand(+ReLU) -> dw3x3(+ReLU) -> pw-project (+residual) (+ReLU)
//   = the reference's BasicResBlock (src/model_training/model/yolo_fastest.py:52-66) and the un-named
//   bottlenecks conv1_2/1_3/1_4, conv2_2/2_3/3_1, conv3_2/3_3/3_4, conv3_5/3_6/4_1, conv4_2/4_3/5_1 (:80-118);
//   with PRE it also evaluates conv0 (dense 3x3 s2 on the 1-channel input, :78) in front of the expansion.  A 1-channel stem first
//   copies the input patch of its region into LDS (f32 planes, u8 frames or 2x u8 frames alike: floats, the pre-process applied once
//   per input pixel) and reads conv0's taps there; the patch shares E's storage.  2 .. 4 input channels fetch every tap from memory.
//
// One workgroup = one spatial tile of one frame.  Data flow per tile:
//   HBM --(narrow NHWC input tile + halo, 16-B loads)--> registers --expand--> LDS (chunk of EC, channel pairs interleaved:
//   expanded channels over the halo'd region) --sliding window--> registers (dw) --> project accumulators in
//   registers --> HBM (narrow NHWC output).  Padding semantics: the depthwise conv pads ITS input, i.e. the
//   expanded tensor is zero outside the image (not relu(bias)).
// All weights are wave-uniform and travel through the scalar path (s_load -> SGPR operand of v_fma_f32).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yf_kernels.h"

// Output pixels per thread (BH x BW) of the two stride-2 / stride-4 VALU blocks: these kernels are LATENCY-bound (47-55 % of their wave
// time parked, profiles/r02_wave_time_breakdown.txt) and their residency is set by the E tile in LDS; 16x32-pixel tiles (1 x 2 per
// thread, 20.7 KB, 7 workgroups per CU) beat 32x32 (2 x 2, 39 KB, 4 per CU) although the halo share of the expansion grows from 13
// to 20 %: stem 70.9 -> 66.8 us, res2 blocks 58 -> 54 us (A/B, tools/ops_ab.sh).  The stem uses 1 x 2; res2 uses 32x16 tiles (2 x 1 per
// thread), another 6 % faster than 16x32 (54 -> 50 us).
// Expansion / projection / conv0 FMAs run over output-channel PAIRS as v_pk_fma_f32 (scalar weight pair x broadcast value).

namespace yf {

constexpr int RES2_BH = 2, RES2_BW = 1;

typedef float fb_f32x2 __attribute__((ext_vector_type(2)));
typedef float __attribute__((address_space(4))) cfloat;               // constant address space: scalar (s_load) reads of uniform data
typedef fb_f32x2 __attribute__((address_space(4))) cfloat2;

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }


// Weight stream of one block (host-packed, fb_pack_weights): per EC-channel chunk, contiguous
//   [W1 chunk CIN x EC | b1 EC | wd 9 x EC | bd EC | W2 chunk EC x COUT], then b2[COUT]
// so that a wave fetches a chunk's weights with a few s_load_dwordx16 instead of strided single-dword loads.
__host__ __device__ constexpr int fb_chunk_floats(int cin, int cout, int ec) { return cin * ec + ec + 9 * ec + ec + ec * cout; }

template <int CIN, int CEXP, int COUT, int S, bool RES, bool RELU_OUT, bool PRE, int TYB, int TXB, int BH, int BW,
          int EC, int CG, int PE, typename T, int C0 = 1>
__global__ void __launch_bounds__(TYB* TXB) fused_block_kernel(FbArgs a)
{
    // C0 (PRE only): input channels of conv0 = io_params input_channel (yolo_fastest.py:78): 1 (gray), 3 (cv2's BGR), or 2 / 4 (NCHW
    // planes; u8 frames: HWC, channel order reversed like `img[:, :, ::-1]`, detect.py:119)
    static_assert(C0 == 1 || (PRE && C0 >= 2 && C0 <= 4), "conv0 on 1 .. 4 input channels");
    constexpr int NT = TYB * TXB, NW = NT / 64;
    constexpr int O_B1 = CIN * EC, O_WD = O_B1 + EC, O_BD = O_WD + 9 * EC, O_W2 = O_BD + EC, CHF = O_W2 + EC * COUT;
    static_assert(CHF == fb_chunk_floats(CIN, COUT, EC), "pack layout");
    constexpr int TH = TYB * BH, TW = TXB * BW;
    constexpr int RH = (TH - 1) * S + 3, RW = (TW - 1) * S + 3;
    constexpr int RWP = (RW + 3) & ~3;            // row pitch (floats), 16-B aligned rows
    constexpr int PLANE = RH * RWP;               // floats per channel (E interleaves channel pairs: [EC/2][RH][RWP][2])
    constexpr int NRP = RH * RW, NPB = (NRP + 64 * PE - 1) / (64 * PE), NCG = EC / CG, NITEM = NPB * NCG;
    constexpr int WR = (BH - 1) * S + 3, WC = (BW - 1) * S + 3;  // dw window of one thread's output block
    static_assert(NT % 64 == 0 && CEXP % EC == 0 && EC % CG == 0 && COUT % 4 == 0, "shape");
    static_assert(!RES || (CIN == COUT && S == 1 && !PRE), "residual needs same shape");
    static_assert(CIN % 4 == 0 || PRE, "NHWC 16-B loads");
    __shared__ __attribute__((aligned(16))) float E[EC * PLANE];
    // u8 input (PRE): (v - 128) / 255 of the 256 possible pixel values (a 2x2 box mean is an integer 0..255 too).  The IEEE division is
    // ~10 VALU instructions and sat in the loop nine times per region pixel (stem 98 us from u8 against 67 us from f32, batch 256); one
    // division per thread here and an LDS read per tap (STAGE: per input pixel) give the same bits (torch's `(img - 128.0) / 255.0`,
    // detect.py:124)
    __shared__ float LUT[PRE ? 256 : 1];

    const int b = xcd_tile(blockIdx.x, gridDim.x);
    const int tx = b % a.tiles_x, ty = (b / a.tiles_x) % a.tiles_y, n = b / (a.tiles_x * a.tiles_y);
    const int oy0 = ty * TH, ox0 = tx * TW, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const int tyb = threadIdx.x / TXB, txb = threadIdx.x % TXB;

    // STAGE (the stem of a 1-channel model): conv0's taps come from a copy of the input patch in LDS.  The region's RH x RW pixels read
    // input rows 2 * iy0 - 1 .. + 2 * RH and columns 2 * ix0 - 1 .. + 2 * RW: each input pixel up to 9/4 times, and fetched per tap every read
    // had its own address arithmetic, bounds test and branch (9 global_load_dword per item under 9 exec masks, an exposed L2 round trip
    // per item; from u8 frames 18 loads and 9 table look-ups).  Staged, a unit of four pixels (16 bytes of an f32 plane, 4 bytes of a u8
    // frame, 2 x 8 bytes of a 2x u8 frame) is loaded once under one predicate -- a unit lies wholly inside its row or wholly outside,
    // and the address of one outside may lie in front of the first frame or behind the last: it is never formed (the load goes to the
    // frame's first unit, not under a branch: a branch per load made the compiler wait for each load before the next); zeros take its
    // place, conv0's padding -- and the table look-up (and the 2x2 box mean) runs once per input pixel.  The patch is stored as floats in two
    // planes per row, [even columns: tap kx = 1 | odd columns: taps kx = 0 and 2] (the split k19r_kernel uses for its slice): a tap's
    // 64 lanes read consecutive dwords at an immediate offset from ONE per-lane base.  All loads are issued before the first LDS write.
    constexpr bool STAGE = PRE && C0 == 1;
    constexpr int PR = 2 * RH + 1, PU = (2 * RW + 5) / 4, PP = 4 * PU;   // patch rows, 4-pixel units per row, row pitch (floats)
    constexpr int NU = PR * PU, UPT = STAGE ? (NU + NT - 1) / NT : 1;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef u32x4 __attribute__((aligned(4))) u32x4_u;   // the caller's frames: no alignment beyond the element's is promised
    typedef u32x2 __attribute__((aligned(1))) u32x2_u;
    typedef unsigned __attribute__((aligned(1))) u32_u;
    u32x4 raw[UPT];
    bool uok[UPT];
    if constexpr (STAGE) {
        static_assert(CEXP == EC && NCG == 1 && PE == 1, "the patch is read before the one chunk's expansion overwrites it");
        static_assert(PR * PP <= EC * PLANE && 2 * PU >= RW + 2 && (TW * S) % 2 == 0, "patch layout");
        static_assert(RWP > RW && (TXB - 1) * BW * S + WC <= RW, "a pad column behind every E row that no depthwise window reads");
        const int IH = 2 * a.H, IW = 2 * a.W;              // the net input's size
        const int py0 = 2 * iy0 - 1, px0 = 2 * ix0 - 2;   // input row / column of the patch's first unit (px0 is a multiple of 4)
        int uy[UPT], ux[UPT];   // the unit's first pixel within frame n; a unit outside the frame reads the frame's first unit instead, as mres_stage does
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const int u = threadIdx.x + k * NT, r = u / PU, yy = py0 + r, xx = px0 + 4 * (u - r * PU);
            uok[k] = u < NU && yy >= 0 && yy < IH && xx >= 0 && xx < IW;
            uy[k] = uok[k] ? yy : 0; ux[k] = uok[k] ? xx : 0;
        }
        if (!a.in_u8) {
            const float* __restrict__ src = a.in + (long)n * IH * IW;
#pragma unroll
            for (int k = 0; k < UPT; ++k) raw[k] = *reinterpret_cast<const u32x4_u*>(src + (uy[k] * IW + ux[k]));
        } else if (!a.u8_down2) {
            const uint8_t* __restrict__ src = a.in_u8 + (long)n * IH * IW;
#pragma unroll
            for (int k = 0; k < UPT; ++k) raw[k] = u32x4{*reinterpret_cast<const u32_u*>(src + (uy[k] * IW + ux[k])), 0u, 0u, 0u};
        } else {   // the 2x2 source blocks of the unit's four pixels: 8 bytes of two source rows
            const uint8_t* __restrict__ src = a.in_u8 + (long)n * 4 * IH * IW;
#pragma unroll
            for (int k = 0; k < UPT; ++k) {
                const uint8_t* q = src + ((long)uy[k] * (2 * IW) + ux[k]) * 2;
                const u32x2 r0 = *reinterpret_cast<const u32x2_u*>(q), r1 = *reinterpret_cast<const u32x2_u*>(q + 2 * IW);
                raw[k] = u32x4{r0.x, r0.y, r1.x, r1.y};
            }
        }
    }
    if constexpr (PRE) {
        if (a.in_u8)
            for (int i = threadIdx.x; i < 256; i += NT) LUT[i] = ((float)i - 128.0f) / 255.0f;
    }
    __syncthreads();   // orders the LUT fill before the look-ups
    if constexpr (STAGE) {
        // Detect_YOLO.__pre_process (src/detect.py:115-124) for u8 frames: optional exact-2x box mean (a+b+c+d+2)>>2, then (v-128)/255;
        // conv0 zero-pads the NORMALISED tensor.  The patch lives in E's storage: the wave's conv0 results wait in registers while a
        // barrier separates the last tap read from the first write of the expansion.
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const int u = threadIdx.x + k * NT, r = u / PU, cu = u - r * PU;
            float v[4];
            if (!a.in_u8) {
                const float4 f = __builtin_bit_cast(float4, raw[k]);
                v[0] = uok[k] ? f.x : 0.f; v[1] = uok[k] ? f.y : 0.f; v[2] = uok[k] ? f.z : 0.f; v[3] = uok[k] ? f.w : 0.f;
            } else if (!a.u8_down2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = uok[k] ? LUT[(raw[k].x >> (8 * j)) & 255u] : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned t0 = raw[k][j / 2] >> (16 * (j & 1)), t1 = raw[k][2 + j / 2] >> (16 * (j & 1));
                    v[j] = uok[k] ? LUT[((t0 & 255u) + ((t0 >> 8) & 255u) + (t1 & 255u) + ((t1 >> 8) & 255u) + 2u) >> 2] : 0.f;
                }
            }
            if (u < NU) {
                *reinterpret_cast<float2*>(E + r * PP + 2 * cu) = make_float2(v[0], v[2]);            // even columns, one slot in
                *reinterpret_cast<float2*>(E + r * PP + 2 * PU + 2 * cu) = make_float2(v[1], v[3]);   // odd columns
            }
        }
        __syncthreads();
    }

    fb_f32x2 acc2[BH * BW][COUT / 2];   // projection accumulators, output-channel pairs
#pragma unroll
    for (int p = 0; p < BH * BW; ++p)
#pragma unroll
        for (int co = 0; co < COUT / 2; ++co) acc2[p][co] = fb_f32x2{0.f, 0.f};

    // HOIST (blocks whose items are whole pixel blocks: res1_1, the res2 pair): a region pixel's input channels do not depend on the
    // chunk, yet the item loop below re-loaded them in every chunk -- and every load was one exposed L2 round trip per item and chunk
    // (load, wait, 16 / 32 packed FMAs, next item).  With HOIST the wave's MAXI items are loaded ONCE, all requests in flight together,
    // before the chunk loop, and stay in registers (MAXI x CIN VGPRs).
    constexpr int MAXI = (NITEM + NW - 1) / NW;
    constexpr bool HOIST = !PRE && NCG == 1 && PE == 1 && MAXI * CIN <= 32;
    float xh[HOIST ? MAXI : 1][CIN];
    int hdst[HOIST ? MAXI : 1];       // ... and so are the item's E offset (-1: no pixel) and its ReLU limit (+inf inside the image, 0 outside):
    float hlim[HOIST ? MAXI : 1];     // 13 of the 64 VALU instructions of an item and chunk were this index arithmetic
    if constexpr (HOIST) {
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int rp = (wave + it * NW) * 64 + lane;      // item = pixel block (NCG == 1, PE == 1); beyond the region: pixel 0, unused
            const int ryh = (rp < NRP ? rp : 0) / RW, rxh = (rp < NRP ? rp : 0) - ryh * RW;
            const int iy = iy0 + ryh, ix = ix0 + rxh;
            const bool in = rp < NRP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            hdst[it] = rp < NRP ? (ryh * RWP + rxh) * 2 : -1;
            hlim[it] = in ? __builtin_inff() : 0.f;
            const T* __restrict__ srch = reinterpret_cast<const T*>(a.in) + (((long)n * a.H + (in ? iy : 0)) * a.W + (in ? ix : 0)) * CIN;
#pragma unroll
            for (int k = 0; k < CIN; k += 4) {
                const float4 t = ld4<T>(srch + k);
                xh[it][k] = t.x; xh[it][k + 1] = t.y; xh[it][k + 2] = t.z; xh[it][k + 3] = t.w;
            }
        }
    }

    for (int ch = 0; ch < CEXP / EC; ++ch) {
        const cfloat* __restrict__ wc = (const cfloat*)(a.wp + ch * CHF);  // this chunk's weights (wave-uniform, constant address space -> scalar loads)
        // ---------------- expansion of the halo'd region into LDS: PE pixels per lane per item ----------------
        if constexpr (STAGE) {
            // two passes over the wave's MAXI items (an item = 64 region pixels): conv0 from the patch, then -- the patch is dead -- the
            // expansion into E.  The compiler still fetches a pass's weights once per item (every item sits under its own wave-uniform
            // guard); with the guard of the first items dropped it keeps them across items and spills SGPRs to VGPR lanes, ~100
            // v_readlane / v_writelane per wave (profiles/stem_lds_taps_ab.txt)
            float x0[MAXI][CIN];
            int dst0[MAXI];       // the pixel's E offset; lanes beyond the region write their zeros into a pad column (RW .. RWP - 1: never read)
            bool in0[MAXI];
#pragma unroll
            for (int it = 0; it < MAXI; ++it) {
                if (wave + it * NW >= NITEM) continue;
                const int rp = (wave + it * NW) * 64 + lane, rpc = rp < NRP ? rp : 0;
                const int ry = rpc / RW, rx = rpc - ry * RW, iy = iy0 + ry, ix = ix0 + rx;
                in0[it] = rp < NRP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                dst0[it] = (ry * RWP + (rp < NRP ? rx : RW)) * 2;
                // conv0: 3x3 stride 2 pad 1 on the net input (+ReLU); v[ky * 3 + kx].  A pixel outside the image reads whatever its taps
                // hold: its expansion is replaced by the depthwise conv's zero padding below
                const float* pt = E + 2 * ry * PP + rx;
                float v[9];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    v[ky * 3] = pt[ky * PP + 2 * PU]; v[ky * 3 + 1] = pt[ky * PP + 1]; v[ky * 3 + 2] = pt[ky * PP + 2 * PU + 1];
                }
#pragma unroll
                for (int c = 0; c < CIN; c += 2) {
                    fb_f32x2 s2 = *(const cfloat2*)(const cfloat*)(a.b0 + c);
#pragma unroll
                    for (int t = 0; t < 9; ++t)
                        s2 = __builtin_elementwise_fma(fb_f32x2{v[t], v[t]}, *(const cfloat2*)(const cfloat*)(a.w0 + t * CIN + c), s2);
                    x0[it][c] = fmaxf(s2[0], 0.f); x0[it][c + 1] = fmaxf(s2[1], 0.f);
                }
            }
            __syncthreads();   // every wave has read its taps: E may be written
#pragma unroll
            for (int it = 0; it < MAXI; ++it) {
                if (wave + it * NW >= NITEM) continue;
                fb_f32x2 e2[CG / 2];
#pragma unroll
                for (int j = 0; j < CG; j += 2) e2[j / 2] = *(const cfloat2*)(wc + O_B1 + j);
#pragma unroll
                for (int k = 0; k < CIN; ++k)
#pragma unroll
                    for (int j = 0; j < CG; j += 2)
                        e2[j / 2] = __builtin_elementwise_fma(fb_f32x2{x0[it][k], x0[it][k]}, *(const cfloat2*)(wc + k * EC + j), e2[j / 2]);
#pragma unroll
                for (int j = 0; j < CG; j += 2)
                    *reinterpret_cast<float2*>(E + dst0[it] + j * PLANE) =
                        make_float2(in0[it] ? fmaxf(e2[j / 2][0], 0.f) : 0.f, in0[it] ? fmaxf(e2[j / 2][1], 0.f) : 0.f);
            }
        } else {
#pragma unroll
        for (int it = 0; it < (HOIST ? MAXI : 1); ++it)   // HOIST: item it of this wave, unrolled so that xh[it] is a register; else the plain item loop
        for (int item = HOIST ? wave + it * NW : wave; item < (HOIST ? (wave + it * NW < NITEM ? wave + it * NW + 1 : 0) : NITEM); item += NW) {
            const int pb = item % NPB, cg = item / NPB;
            float x[PE][CIN];
            int ry[PE], rx[PE];
            bool inreg[PE], inimg[PE];
#pragma unroll
            for (int p = 0; p < PE; ++p) {
                const int rp = pb * (64 * PE) + p * 64 + lane;
                ry[p] = rp / RW; rx[p] = rp - ry[p] * RW;
                const int iy = iy0 + ry[p], ix = ix0 + rx[p];
                inreg[p] = rp < NRP;
                inimg[p] = inreg[p] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                if constexpr (PRE) {
                    // conv0: 3x3 stride 2 pad 1 on the C0-channel net input (+ReLU); v[(ky * 3 + kx) * C0 + ci]
                    float v[9 * C0];
                    if (a.in_u8) {
                        // Detect_YOLO.__pre_process fused into the load (src/detect.py:115-124): u8 gray frame, optional
                        // exact-2x box mean (a+b+c+d+2)>>2, then (v-128)/255; conv0 zero-pads the NORMALISED tensor
                        // (C0 = 3: the frame is cv2's HWC BGR; net channel ci is source channel 2 - ci, detect.py:119)
                        // Branch-free and in two passes: ALL byte loads of the 9 C0 taps first (from addresses clamped into the frame, so no
                        // load sits under a bounds branch), the table look-ups after, zeros selected in at the end.  Written tap by tap
                        // (bounds branch, load, look up) the compiler waited for every load before its look-up: nine dependent memory
                        // round trips per region pixel (stem 84 us from u8 against 66 us from f32).
                        const int sw = (a.u8_down2 ? 4 * a.W : 2 * a.W) * C0;
                        const uint8_t* __restrict__ src = a.in_u8 + (long)n * (a.u8_down2 ? 16L : 4L) * a.H * a.W * C0;
                        int yo[3], xo[3];
                        unsigned rows = 0, cols = 0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int yy = 2 * iy - 1 + k, xx = 2 * ix - 1 + k;
                            const int yc = min(max(yy, 0), 2 * a.H - 1), xc = min(max(xx, 0), 2 * a.W - 1);
                            yo[k] = (a.u8_down2 ? 2 * yc : yc) * sw;
                            xo[k] = (a.u8_down2 ? 2 * xc : xc) * C0;
                            if (inimg[p] && yy == yc) rows |= 0x7u << (3 * k);      // tap row k inside the frame
                            if (xx == xc) cols |= 0x49u << k;                        // tap column k inside the frame
                        }
                        const unsigned okm = rows & cols;   // bit ky * 3 + kx: the tap reads the image (else conv0's zero padding)
                        if (a.u8_down2) {
                            unsigned r0[9 * C0], r1[9 * C0];   // the two source rows of a tap's 2x2 block: two pixels each
#pragma unroll
                            for (int t = 0; t < 9 * C0; ++t) {
                                const uint8_t* q = src + yo[t / C0 / 3] + xo[(t / C0) % 3] + (C0 - 1 - t % C0);
                                r0[t] = (unsigned)q[0] | ((unsigned)q[C0] << 8);
                                r1[t] = (unsigned)q[sw] | ((unsigned)q[sw + C0] << 8);
                            }
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int t = 0; t < 9 * C0; ++t) {
                                const float lv = LUT[((r0[t] & 255u) + (r0[t] >> 8) + (r1[t] & 255u) + (r1[t] >> 8) + 2u) >> 2];
                                v[t] = (okm >> (t / C0)) & 1u ? lv : 0.f;
                            }
                        } else {
                            unsigned r0[9 * C0];
#pragma unroll
                            for (int t = 0; t < 9 * C0; ++t) r0[t] = src[yo[t / C0 / 3] + xo[(t / C0) % 3] + (C0 - 1 - t % C0)];
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int t = 0; t < 9 * C0; ++t) {
                                const float lv = LUT[r0[t]];
                                v[t] = (okm >> (t / C0)) & 1u ? lv : 0.f;
                            }
                        }
                    } else {
                        const long plane = 4L * a.H * a.W;   // NCHW input: C0 planes per frame
                        const float* __restrict__ src = a.in + (long)n * C0 * plane;
#pragma unroll
                        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) {
                                int yy = 2 * iy - 1 + ky, xx = 2 * ix - 1 + kx;
                                bool ok = inimg[p] && yy >= 0 && yy < 2 * a.H && xx >= 0 && xx < 2 * a.W;
#pragma unroll
                                for (int ci = 0; ci < C0; ++ci) v[(ky * 3 + kx) * C0 + ci] = ok ? src[ci * plane + (long)yy * (2 * a.W) + xx] : 0.f;
                            }
                    }
#pragma unroll
                    for (int c = 0; c < CIN; c += 2) {
                        fb_f32x2 s2 = *(const cfloat2*)(const cfloat*)(a.b0 + c);
#pragma unroll
                        for (int t = 0; t < 9 * C0; ++t)
                            s2 = __builtin_elementwise_fma(fb_f32x2{v[t], v[t]}, *(const cfloat2*)(const cfloat*)(a.w0 + t * CIN + c), s2);
                        x[p][c] = fmaxf(s2[0], 0.f); x[p][c + 1] = fmaxf(s2[1], 0.f);
                    }
                } else if constexpr (HOIST) {
#pragma unroll
                    for (int k = 0; k < CIN; ++k) x[p][k] = xh[it][k];
                } else {
                    const T* __restrict__ src = reinterpret_cast<const T*>(a.in) + (((long)n * a.H + (inimg[p] ? iy : 0)) * a.W + (inimg[p] ? ix : 0)) * CIN;
#pragma unroll
                    for (int k = 0; k < CIN; k += 4) {
                        float4 t = ld4<T>(src + k);
                        x[p][k] = t.x; x[p][k + 1] = t.y; x[p][k + 2] = t.z; x[p][k + 3] = t.w;
                    }
                }
            }
            float e[PE][CG];
            static_assert(CG % 2 == 0 && EC % 2 == 0, "channel pairs");
            fb_f32x2 e2[PE][CG / 2];
#pragma unroll
            for (int j = 0; j < CG; j += 2) {
                const fb_f32x2 bv = *(const cfloat2*)(wc + O_B1 + cg * CG + j);
#pragma unroll
                for (int p = 0; p < PE; ++p) e2[p][j / 2] = bv;
            }
#pragma unroll
            for (int k = 0; k < CIN; ++k)
#pragma unroll
                for (int j = 0; j < CG; j += 2) {
                    const fb_f32x2 wv = *(const cfloat2*)(wc + k * EC + cg * CG + j);
#pragma unroll
                    for (int p = 0; p < PE; ++p) e2[p][j / 2] = __builtin_elementwise_fma(fb_f32x2{x[p][k], x[p][k]}, wv, e2[p][j / 2]);
                }
#pragma unroll
            for (int p = 0; p < PE; ++p)
#pragma unroll
                for (int j = 0; j < CG; ++j) e[p][j] = e2[p][j / 2][j & 1];
            // E holds channel PAIRS interleaved: [EC/2][RH][RWP][2] -- one 8-byte write per pair here, and the depthwise below runs
            // its taps on both channels of a pair with one v_pk_fma_f32
#pragma unroll
            for (int p = 0; p < PE; ++p)
                if (HOIST ? hdst[it] >= 0 : inreg[p]) {
                    float* dst = E + (cg * CG) * PLANE + (HOIST ? hdst[it] : (ry[p] * RWP + rx[p]) * 2);
                    // ReLU and the zero outside the image in ONE instruction per value: median(x, 0, lim), lim = +inf inside, 0 outside
                    // (v_max + v_cndmask before: 2 of every ~7 VALU instructions of the res2 expansion: res2_1 / res2_2 40.2 -> 36.7 us; not in the
                    //  stem, which it slows from 57.7 to 62.1 us -- A/B, tools/ops_abn.sh)
                    const float lim = HOIST ? hlim[it] : inimg[p] ? __builtin_inff() : 0.f;
#pragma unroll
                    for (int j = 0; j < CG; j += 2)
                        *reinterpret_cast<float2*>(dst + j * PLANE) =
                            !PRE ? make_float2(__builtin_amdgcn_fmed3f(e[p][j], 0.f, lim), __builtin_amdgcn_fmed3f(e[p][j + 1], 0.f, lim))
                                       : make_float2(inimg[p] ? fmaxf(e[p][j], 0.f) : 0.f, inimg[p] ? fmaxf(e[p][j + 1], 0.f) : 0.f);
                }
        }
        }
        __syncthreads();
        // ---------------- depthwise 3x3 from LDS + projection into registers ----------------
        // NOT fully unrolled: unrolled, the scalar loads of all EC channels' weights are hoisted to the top and, with the
        // expansion's, exceed the SGPR file -- the compiler then spills SGPRs to VGPR lanes and 30-50 % of the VALU
        // instructions of the stride-2 kernels were v_readlane / v_writelane (tools/isa_stats.py)
#pragma unroll 1
        for (int c = 0; c < EC; c += 2) {
            const float* Ec = E + c * PLANE + ((tyb * BH * S) * RWP + txb * BW * S) * 2;
            fb_f32x2 win[WR][WC];   // (channel c, channel c + 1) of every window pixel
#pragma unroll
            for (int r = 0; r < WR; ++r) {
                if constexpr ((BW * S) % 2 == 0) {   // 16-byte aligned: two pixels x two channels per read
#pragma unroll
                    for (int q = 0; q + 1 < WC; q += 2) {
                        const float4 t = *reinterpret_cast<const float4*>(Ec + (r * RWP + q) * 2);
                        win[r][q] = fb_f32x2{t.x, t.y}; win[r][q + 1] = fb_f32x2{t.z, t.w};
                    }
                    if constexpr (WC % 2) win[r][WC - 1] = *reinterpret_cast<const fb_f32x2*>(Ec + (r * RWP + WC - 1) * 2);
                } else {
#pragma unroll
                    for (int q = 0; q < WC; ++q) win[r][q] = *reinterpret_cast<const fb_f32x2*>(Ec + (r * RWP + q) * 2);
                }
            }
            fb_f32x2 wd[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) wd[t] = *(const cfloat2*)(wc + O_WD + t * EC + c);
            const fb_f32x2 bd = *(const cfloat2*)(wc + O_BD + c);
#pragma unroll
            for (int by = 0; by < BH; ++by)
#pragma unroll
                for (int bx = 0; bx < BW; ++bx) {
                    fb_f32x2 d2 = bd;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) d2 = __builtin_elementwise_fma(win[by * S + ky][bx * S + kx], wd[ky * 3 + kx], d2);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float d = fmaxf(d2[h], 0.f);
#pragma unroll
                        for (int co = 0; co < COUT; co += 2)
                            acc2[by * BW + bx][co / 2] = __builtin_elementwise_fma(fb_f32x2{d, d}, *(const cfloat2*)(wc + O_W2 + (c + h) * COUT + co),
                                                                                    acc2[by * BW + bx][co / 2]);
                    }
                }
        }
        __syncthreads();
    }
    // ---------------- epilogue: bias (+ residual) (+ ReLU), NHWC store ----------------
    const cfloat* __restrict__ b2 = (const cfloat*)(a.wp + (CEXP / EC) * CHF);
#pragma unroll
    for (int by = 0; by < BH; ++by)
#pragma unroll
        for (int bx = 0; bx < BW; ++bx) {
            const int oy = oy0 + tyb * BH + by, ox = ox0 + txb * BW + bx;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const long opix = ((long)n * a.Ho + oy) * a.Wo + ox;
            T* o = reinterpret_cast<T*>(a.out) + opix * COUT;
#pragma unroll
            for (int co = 0; co < COUT; co += 4) {
                float4 v = make_float4(acc2[by * BW + bx][co / 2][0] + b2[co], acc2[by * BW + bx][co / 2][1] + b2[co + 1],
                                       acc2[by * BW + bx][co / 2 + 1][0] + b2[co + 2], acc2[by * BW + bx][co / 2 + 1][1] + b2[co + 3]);
                if constexpr (RES) {
                    float4 r = ld4<T>(reinterpret_cast<const T*>(a.in) + opix * CIN + co);
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                if constexpr (RELU_OUT) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                st4<T>(o + co, v);
            }
        }
}

// ------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------
template <int CIN, int CEXP, int COUT, int S, bool RES, bool RELU_OUT, bool PRE, int TYB, int TXB, int BH, int BW, int EC, int CG, int PE, typename T, int C0 = 1>
static int launch_fb_t(FbArgs a, int N, hipStream_t s)
{
    a.tiles_y = (a.Ho + TYB * BH - 1) / (TYB * BH);
    a.tiles_x = (a.Wo + TXB * BW - 1) / (TXB * BW);
    dim3 grid((unsigned)(N * a.tiles_y * a.tiles_x));
    hipLaunchKernelGGL((fused_block_kernel<CIN, CEXP, COUT, S, RES, RELU_OUT, PRE, TYB, TXB, BH, BW, EC, CG, PE, T, C0>), grid,
                       dim3(TYB * TXB), 0, s, a);
    return 0;
}

// (Staging the NHWC block input in LDS was measured slower at these shapes: one use per pixel, it costs occupancy and LDS bandwidth, the
//  L2-served loads were already hidden.  The stem's net input is another matter: nine uses per pixel, staged in E's own storage -- STAGE above.)
//     cin cexp cout S  res    relu   pre    TYB TXB BH BW EC CG PE
#define YF_FB_SHAPES(FB)                                                                                                 \
    FB(8, 8, 4, 1, false, false, true, 16, 16, 1, 2, 8, 8, 1)            /* conv0 + conv1_2/1_3/1_4      @ H/2  */          \
    FB(8, 8, 4, 1, false, false, false, 16, 16, 1, 2, 8, 8, 1)           /* conv1_2/1_3/1_4 behind a separate conv0 (input_channel > 4) */ \
    FB(4, 8, 4, 1, true, false, false, 16, 16, 1, 2, 8, 8, 1)            /* res1_1                        @ H/2  */          \
    FB(8, 32, 8, 1, true, false, false, 16, 16, RES2_BH, RES2_BW, 8, 8, 1)                 /* res2_1, res2_2                @ H/4  */          \
    FB(8, 32, 8, 2, false, false, false, 16, 20, 1, 1, 8, 8, 1)          /* conv2_2/2_3/3_1               H/4 -> H/8 */      \
    FB(8, 48, 8, 1, true, false, false, 16, 20, 1, 2, 8, 8, 2)           /* res3_1, res3_2                @ H/8  */          \
    FB(8, 48, 16, 1, false, false, false, 16, 20, 1, 2, 8, 8, 2)         /* conv3_2/3_3/3_4 (fallback)    @ H/8  */          \
    FB(16, 96, 16, 1, true, false, false, 16, 20, 1, 2, 8, 8, 1)         /* res3_3 .. res3_6 (fallback)   @ H/8  */          \
    FB(16, 96, 24, 2, false, false, false, 16, 20, 1, 1, 8, 8, 1)        /* conv3_5/3_6/4_1               H/8 -> H/16 */     \
    FB(24, 136, 24, 1, true, false, false, 16, 20, 1, 1, 8, 8, 1)        /* res4_1 .. res4_4 (fallback)   @ H/16 */

int launch_fused_block(int cin, int cexp, int cout, int stride, bool res, bool relu_out, int pre_c0, const FbArgs& a, int N,
                       hipStream_t s, int dtype)
{
    const bool pre = pre_c0 != 0;
    if (pre && (pre_c0 < 1 || pre_c0 > 4)) return -1;
    if (pre_c0 > 1) {   // the stem of a multi-channel model: the same tile shape, conv0 over C0 input planes
        if (!(cin == 8 && cexp == 8 && cout == 4 && stride == 1 && !res && !relu_out)) return -1;
#define YF_STEM_C0(C0_)                                                                                                                            \
        if (pre_c0 == C0_)                                                                                                                          \
            return dtype == DT_F16 ? launch_fb_t<8, 8, 4, 1, false, false, true, 16, 16, 1, 2, 8, 8, 1, half_t, C0_>(a, N, s) \
                                   : launch_fb_t<8, 8, 4, 1, false, false, true, 16, 16, 1, 2, 8, 8, 1, float, C0_>(a, N, s);
        YF_STEM_C0(2) YF_STEM_C0(3) YF_STEM_C0(4)
#undef YF_STEM_C0
        return -1;
    }
    // Small batches (round 5): the res2 blocks (stride 4: 80x64 pixels per frame of the 320x256 net) on 16x16 tiles instead of 32x16 when the
    // larger tiling would leave more than half of the CUs idle -- one output pixel per lane instead of two; a pixel's arithmetic is the same.
    if (cin == 8 && cexp == 32 && cout == 8 && stride == 1 && res && !relu_out && !pre) {
        const int n_cu = device_cu_count(current_device());
        const long big = (long)N * ((a.Ho + 16 * RES2_BH - 1) / (16 * RES2_BH)) * ((a.Wo + 16 * RES2_BW - 1) / (16 * RES2_BW));
        if (n_cu > 0 && 2 * big <= n_cu)
            return dtype == DT_F16 ? launch_fb_t<8, 32, 8, 1, true, false, false, 16, 16, 1, 1, 8, 8, 1, half_t>(a, N, s)
                                   : launch_fb_t<8, 32, 8, 1, true, false, false, 16, 16, 1, 1, 8, 8, 1, float>(a, N, s);
    }
#define FB(ci, ce, co, st, rs, ro, pr, tyb, txb, bh, bw, ec, cg, pe)                                              \
    if (cin == ci && cexp == ce && cout == co && stride == st && res == rs && relu_out == ro && pre == pr)         \
        return dtype == DT_F16 ? launch_fb_t<ci, ce, co, st, rs, ro, pr, tyb, txb, bh, bw, ec, cg, pe, half_t>(a, N, s)       \
                               : launch_fb_t<ci, ce, co, st, rs, ro, pr, tyb, txb, bh, bw, ec, cg, pe, float>(a, N, s);
    YF_FB_SHAPES(FB)
#undef FB
    return -1;
}

int fb_chunk_channels(int cin, int cexp, int cout, int stride, bool res, bool relu_out, int pre_c0)
{
    const bool pre = pre_c0 != 0;
#define FB(ci, ce, co, st, rs, ro, pr, tyb, txb, bh, bw, ec, cg, pe) \
    if (cin == ci && cexp == ce && cout == co && stride == st && res == rs && relu_out == ro && pre == pr) return ec;
    YF_FB_SHAPES(FB)
#undef FB
    return -1;
}

size_t fb_packed_floats(int cin, int cexp, int cout, int ec) { return (size_t)(cexp / ec) * fb_chunk_floats(cin, cout, ec) + cout; }

void fb_pack_weights(const float* w1 /*[cin][cexp]*/, const float* b1, const float* wd /*[9][cexp]*/, const float* bd,
                     const float* w2 /*[cexp][cout]*/, const float* b2, int cin, int cexp, int cout, int ec, float* out)
{
    const int CHF = fb_chunk_floats(cin, cout, ec);
    for (int ch = 0; ch < cexp / ec; ++ch) {
        float* o = out + (size_t)ch * CHF;
        for (int k = 0; k < cin; ++k)
            for (int j = 0; j < ec; ++j) o[k * ec + j] = w1[(size_t)k * cexp + ch * ec + j];
        o += cin * ec;
        for (int j = 0; j < ec; ++j) o[j] = b1[ch * ec + j];
        o += ec;
        for (int t = 0; t < 9; ++t)
            for (int j = 0; j < ec; ++j) o[t * ec + j] = wd[(size_t)t * cexp + ch * ec + j];
        o += 9 * ec;
        for (int j = 0; j < ec; ++j) o[j] = bd[ch * ec + j];
        o += ec;
        for (int j = 0; j < ec; ++j)
            for (int co = 0; co < cout; ++co) o[j * cout + co] = w2[(size_t)(ch * ec + j) * cout + co];
    }
    for (int co = 0; co < cout; ++co) out[(size_t)(cexp / ec) * CHF + co] = b2[co];
}

}  // namespace yf
