// yf_jpeg_enc_kernels.hip -- baseline JPEG encoding of uint8 device frames, byte for byte the file PIL (libjpeg-turbo) writes for
// Image.save(f, "JPEG", quality=q, subsampling=s), and plot_one_box's rectangles and label text drawn on device frames.
//   host (yf_jpeg_enc_setup): the header libjpeg writes for these arguments (SOI, JFIF APP0, one DQT per table, SOF0, one DHT per Annex K
//     table, SOS), the quality-scaled quantisation tables as the divisors 8 * q in natural order with 32-bit reciprocals, and the frame
//     geometry, in one small blob.  No GPU call.  The blob travels to the kernels by value as a launch argument: nothing to upload.
//   jpeg_enc_blocks_kernel: one thread per 8x8 block with the block in registers.  rgb_ycc_convert's 16-bit tables, edge replication and
//     h2v2 / h2v1 downsampling as jcprepct.c / jcsample.c order them (input columns and the odd input row replicated before the mean,
//     downsampled rows after it), jfdctint.c's two passes, quantisation (|v| + d / 2) / d through umulhi with the sign put back; int16
//     coefficients in zig-zag order at the block's place in the scan.  A luma block of an MCU outside the luma plane's own blocks is
//     libjpeg's dummy block: zeros with the DC of the block it copies (jccoefct.c).
//   jpeg_enc_lengths_kernel: one thread per block of the scan: its code length in bits (DC difference against the block before it of the
//     same component, AC run / size with ZRL and EOB).
//   jpeg_enc_offsets_kernel: one workgroup per frame: exclusive prefix sum of the lengths in place, the frame's total.
//   jpeg_enc_bits_kernel: one thread per block writes its codes at its bit offset into the frame's unstuffed stream (big-endian 32-bit
//     words, zeroed before): words the block covers whole are stored plainly, the first and last with an integer atomicOr, whose result
//     does not depend on arrival order.
//   jpeg_enc_stuff_kernel: one workgroup per frame: pads the last byte with one-bits, counts the 0xFF bytes (so the file's length is known
//     before a byte is written: a frame that does not fit its slot gets status 1, its needed length, and no byte), then copies header,
//     stream with 0x00 after every 0xFF (prefix sum per tile of 4096 bytes) and EOI into the slot.
//   draw_boxes_kernel: one thread per pixel applies its frame's records in order: five clipped integer rectangles (four edges, label
//     box), then the label's coverage mask with PIL's 8-bit blend  t = d * (255 - m) + ink * m + 128; ((t >> 8) + t) >> 8.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

constexpr uint32_t ENC_MAGIC = 0x31434E45u;       // "ENC1"
constexpr int ENC_MAX_DIM = 8192;
constexpr int ENC_HEADER_CAP = 640;               // 623 bytes for three components
constexpr int ENC_BLOCK_BITS = 1664;              // a block's codes at most: DC 11 + 11, 63 x (16 + 10) AC = 1660 bits, rounded to whole words
constexpr int ENC_TILE = 1024;                    // threads of the per-frame kernels

// ITU-T T.81 Annex K: K.1 (quantisation, zig-zag order as DQT carries them), K.3 (Huffman)
constexpr uint8_t K_Q[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t K_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t K_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t K_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t K_AC_VALS[2][162] = {
    {1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36, 51, 98,
     114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87,
     88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146,
     147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
     195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234,
     241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114,
     209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85,
     86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136,
     137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
     185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232,
     233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
constexpr int ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// (size << 16) | code per symbol: tables 0, 1 = DC luma, chroma; 2, 3 = AC luma, chroma (jpeg_make_c_derived_tbl)
struct HuffEnc {
    uint32_t e[4][256];
};
constexpr HuffEnc make_huff()
{
    HuffEnc t{};
    for (int k = 0; k < 4; ++k) {
        const uint8_t* bits = k < 2 ? K_DC_BITS[k] : K_AC_BITS[k - 2];
        const uint8_t* vals = k < 2 ? K_DC_VALS : K_AC_VALS[k - 2];
        uint32_t code = 0;
        int p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int i = 0; i < bits[l - 1]; ++i) t.e[k][vals[p++]] = ((uint32_t)l << 16) | code++;
            code <<= 1;
        }
    }
    return t;
}
__constant__ HuffEnc g_huff = make_huff();

struct JEnc {                                     // the blob of yf_jpeg_enc_setup, and the kernels' argument
    uint32_t magic;
    int32_t h, w, ncomp, hs, vs, quality;         // hs, vs: luma sampling (chroma is 1 x 1)
    int32_t hdr_len;
    int32_t mcu_rows, mcu_cols, bpm, nblocks;     // blocks per MCU, blocks of the scan per frame
    uint32_t words_cap;                           // 32-bit words of a frame's unstuffed stream
    uint16_t div[2][64];                          // 8 * q, natural order
    uint32_t rcp[2][64];                          // floor(2^32 / div) + 1: (a * rcp) >> 32 == a / div for a < 2^16
    uint8_t header[ENC_HEADER_CAP];
};
static_assert(sizeof(JEnc) <= 2048, "JEnc travels as a kernel argument");

struct EncWs {                                    // offsets into the workspace, 256-byte aligned
    size_t coef, off, total, bits, end;
};
EncWs enc_ws(const JEnc& P, int n)
{
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    EncWs s;
    s.coef = 0;
    s.off = up(s.coef + (size_t)n * P.nblocks * 128);
    s.total = up(s.off + (size_t)n * P.nblocks * 4);
    s.bits = up(s.total + (size_t)n * 4);
    s.end = up(s.bits + (size_t)n * P.words_cap * 4);
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// blocks

__device__ __forceinline__ void px_rgb(const uint8_t* __restrict__ img, int w, int y, int x, int bgr, int& r, int& g, int& b)
{
    const uint8_t* p = img + ((size_t)y * w + x) * 3;
    r = p[bgr ? 2 : 0];
    g = p[1];
    b = p[bgr ? 0 : 2];
}
__device__ __forceinline__ int ycc(int c, int r, int g, int b)
{
    if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ img, int w, int y, int x, int bgr, int c)
{
    int r, g, b;
    px_rgb(img, w, y, x, bgr, r, g, b);
    return ycc(c, r, g, b);
}

// the level-shifted samples of block (by, bx) of component c
__device__ __forceinline__ void load_block(const JEnc& P, const uint8_t* __restrict__ img, int bgr, int c, int by, int bx, int (&d)[64])
{
    const int h = P.h, w = P.w;
    if (P.ncomp == 1 || c == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int y = min(by * 8 + i, h - 1);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int x = min(bx * 8 + j, w - 1);
                int v;
                if (P.ncomp == 1) {
                    v = img[(size_t)y * w + x];
                } else {
                    int r, g, b;
                    px_rgb(img, w, y, x, bgr, r, g, b);
                    v = ycc(0, r, g, b);
                }
                d[i * 8 + j] = v - 128;
            }
        }
        return;
    }
    const int hs = P.hs, vs = P.vs;
    const int ch = (h + vs - 1) / vs;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int cy = min(by * 8 + i, ch - 1);                       // downsampled rows are replicated
        const int y0 = cy * vs, y1 = min(y0 + vs - 1, h - 1);         // the odd input row is replicated before the mean
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int cx = bx * 8 + j;
            const int x0 = min(cx * hs, w - 1), x1 = min(cx * hs + hs - 1, w - 1);   // input columns are replicated before the mean
            int v = chroma_at(img, w, y0, x0, bgr, c);
            if (hs == 2) {
                v += chroma_at(img, w, y0, x1, bgr, c);
                if (vs == 2)
                    v = (v + chroma_at(img, w, y1, x0, bgr, c) + chroma_at(img, w, y1, x1, bgr, c) + 1 + (cx & 1)) >> 2;
                else
                    v = (v + (cx & 1)) >> 1;
            }
            d[i * 8 + j] = v - 128;
        }
    }
}

#define ENC_DESCALE(x, n) (((x) + (1 << ((n)-1))) >> (n))
// one jfdctint.c pass over 8 values at stride S from d[o]
template <int S, bool FIRST>
__device__ __forceinline__ void fdct_1d(int (&d)[64], int o)
{
    constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
    constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[o] + d[o + 7 * S], t7 = d[o] - d[o + 7 * S], t1 = d[o + S] + d[o + 6 * S], t6 = d[o + S] - d[o + 6 * S];
    const int t2 = d[o + 2 * S] + d[o + 5 * S], t5 = d[o + 2 * S] - d[o + 5 * S], t3 = d[o + 3 * S] + d[o + 4 * S], t4 = d[o + 3 * S] - d[o + 4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[o] = (t10 + t11) << 2;
        d[o + 4 * S] = (t10 - t11) << 2;
    } else {
        d[o] = ENC_DESCALE(t10 + t11, 2);
        d[o + 4 * S] = ENC_DESCALE(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * F_0_541;
    d[o + 2 * S] = ENC_DESCALE(z1 + t13 * F_0_765, N);
    d[o + 6 * S] = ENC_DESCALE(z1 - t12 * F_1_847, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175;
    const int u4 = t4 * F_0_298, u5 = t5 * F_2_053, u6 = t6 * F_3_072, u7 = t7 * F_1_501;
    z1 = -z1 * F_0_899;
    z2 = -z2 * F_2_562;
    z3 = -z3 * F_1_961 + z5;
    z4 = -z4 * F_0_390 + z5;
    d[o + 7 * S] = ENC_DESCALE(u4 + z1 + z3, N);
    d[o + 5 * S] = ENC_DESCALE(u5 + z2 + z4, N);
    d[o + 3 * S] = ENC_DESCALE(u6 + z2 + z3, N);
    d[o + S] = ENC_DESCALE(u7 + z1 + z4, N);
}

__device__ __forceinline__ int quant(int v, uint32_t dv, uint32_t rc)
{
    const uint32_t a = (uint32_t)abs(v) + (dv >> 1);
    const int q = (int)__umulhi(a, rc);
    return v < 0 ? -q : q;
}

__global__ __launch_bounds__(256) void jpeg_enc_blocks_kernel(const JEnc P, const uint8_t* __restrict__ frames, int bgr, int16_t* __restrict__ coef)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P.nblocks) return;       // every block of the scan is one block of a component's MCU-padded plane
    const int f = blockIdx.y;
    const uint8_t* img = frames + (size_t)f * P.h * P.w * P.ncomp;
    // component planes, MCU-padded: luma first
    const int ny = P.mcu_rows * P.vs * P.mcu_cols * P.hs, nc = P.mcu_rows * P.mcu_cols;
    int c = 0, r = t;
    if (P.ncomp == 3 && t >= ny) {
        c = 1 + (t - ny) / nc;
        r = (t - ny) % nc;
    }
    const int chs = c == 0 && P.ncomp == 3 ? P.hs : 1, cvs = c == 0 && P.ncomp == 3 ? P.vs : 1;
    const int pw = P.mcu_cols * chs;
    const int by = r / pw, bx = r % pw;
    const int mcu = (by / cvs) * P.mcu_cols + bx / chs;
    const int k = (c == 0 ? 0 : P.hs * P.vs + c - 1) + (by % cvs) * chs + bx % chs;
    int16_t* out = coef + ((size_t)f * P.nblocks + (size_t)mcu * P.bpm + k) * 64;
    // the component's own blocks
    const int cw = c == 0 ? P.w : (P.w + P.hs - 1) / P.hs, chh = c == 0 ? P.h : (P.h + P.vs - 1) / P.vs;
    const int wib = (cw + 7) / 8, hib = (chh + 7) / 8;
    const int tab = c ? 1 : 0;
    int d[64];
    if (by >= hib || bx >= wib) {                  // libjpeg's dummy block: zeros with the DC of the block it copies
        int sy = by, sx = bx - 1;                  // right edge: the block before
        if (by >= hib) {                           // bottom edge: the MCU's last block of the row of blocks above
            sy = by - 1;
            sx = (bx / chs) * chs + chs - 1;
            if (sx >= wib) sx -= 1;                // itself a dummy of the right edge
        }
        load_block(P, img, bgr, c, sy, sx, d);
        int s = 0;
#pragma unroll
        for (int i = 0; i < 64; ++i) s += d[i];    // jfdctint's DC is exactly the sum of the level-shifted samples
        const int dc = quant(s, P.div[tab][0], P.rcp[tab][0]);
        uint4 z = {0, 0, 0, 0};
        uint4 first = {(uint32_t)(uint16_t)dc, 0, 0, 0};
        uint4* o4 = reinterpret_cast<uint4*>(out);
        o4[0] = first;
#pragma unroll
        for (int i = 1; i < 8; ++i) o4[i] = z;
        return;
    }
    load_block(P, img, bgr, c, by, bx, d);
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct_1d<1, true>(d, i * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct_1d<8, false>(d, i);
    uint32_t pk[32];
#pragma unroll
    for (int k2 = 0; k2 < 64; k2 += 2) {
        const int a = ZIGZAG[k2], b = ZIGZAG[k2 + 1];
        const int qa = quant(d[a], P.div[tab][a], P.rcp[tab][a]), qb = quant(d[b], P.div[tab][b], P.rcp[tab][b]);
        pk[k2 / 2] = (uint32_t)(uint16_t)qa | ((uint32_t)(uint16_t)qb << 16);
    }
    uint4* o4 = reinterpret_cast<uint4*>(out);
#pragma unroll
    for (int i = 0; i < 8; ++i) o4[i] = make_uint4(pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// entropy coding

__device__ __forceinline__ int nbits_of(int v) { return 32 - __clz(abs(v)); }      // __clz(0) = 32

// walks one block of the scan: emit(code bits, length) for every code, in order
template <class Emit>
__device__ __forceinline__ void code_block(const JEnc& P, const int16_t* __restrict__ coef, int blk, const uint32_t (*huff)[256], Emit&& emit)
{
    const int k = blk % P.bpm, mcu = blk / P.bpm;
    const int ny = P.ncomp == 3 ? P.hs * P.vs : 1;
    const int tab = k >= ny ? 1 : 0;
    int pred = 0;                                  // the DC of the block before of the same component
    if (k > 0 && k < ny)
        pred = coef[(size_t)(blk - 1) * 64];
    else if (mcu > 0)
        pred = coef[(size_t)(blk - P.bpm + (k == 0 ? ny - 1 : 0)) * 64];
    uint32_t v[32];
    const uint4* c4 = reinterpret_cast<const uint4*>(coef + (size_t)blk * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 q = c4[i];
        v[4 * i] = q.x, v[4 * i + 1] = q.y, v[4 * i + 2] = q.z, v[4 * i + 3] = q.w;
    }
    const int diff = (int)(int16_t)(v[0] & 0xFFFF) - pred;
    int n = nbits_of(diff);
    uint32_t e = huff[tab][n];
    emit(((e & 0xFFFF) << n) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1)), (int)(e >> 16) + n);
    int run = 0;
    const uint32_t zrl = huff[2 + tab][0xF0];
#pragma unroll
    for (int i = 1; i < 64; ++i) {
        const int a = (int)(int16_t)((i & 1) ? v[i / 2] >> 16 : v[i / 2] & 0xFFFF);
        if (a == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            emit(zrl & 0xFFFF, (int)(zrl >> 16));
            run -= 16;
        }
        n = nbits_of(a);
        e = huff[2 + tab][(run << 4) | n];
        emit(((e & 0xFFFF) << n) | ((uint32_t)(a < 0 ? a - 1 : a) & ((1u << n) - 1)), (int)(e >> 16) + n);
        run = 0;
    }
    if (run > 0) {
        e = huff[2 + tab][0];
        emit(e & 0xFFFF, (int)(e >> 16));
    }
}

__device__ __forceinline__ void load_huff(uint32_t (*huff)[256])
{
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) huff[i >> 8][i & 255] = g_huff.e[i >> 8][i & 255];
    __syncthreads();
}

__global__ __launch_bounds__(256) void jpeg_enc_lengths_kernel(const JEnc P, const int16_t* __restrict__ coef, uint32_t* __restrict__ off)
{
    __shared__ uint32_t huff[4][256];
    load_huff(huff);
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= P.nblocks) return;
    const int f = blockIdx.y;
    uint32_t total = 0;
    code_block(P, coef + (size_t)f * P.nblocks * 64, blk, huff, [&](uint32_t, int len) { total += len; });
    off[(size_t)f * P.nblocks + blk] = total;
}

// exclusive prefix sum over the workgroup's ENC_TILE threads; `total` = the sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sh, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(inc, s, 64);
        if (lane >= s) inc += o;
    }
    __syncthreads();                               // sh may still be read from the call before
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < ENC_TILE / 64; ++i) {
        const uint32_t s = sh[i];
        before += i < wv ? s : 0;
        all += s;
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(ENC_TILE) void jpeg_enc_offsets_kernel(const JEnc P, uint32_t* __restrict__ off, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t sh[ENC_TILE / 64];
    uint32_t* o = off + (size_t)blockIdx.x * P.nblocks;
    const int per = (P.nblocks + ENC_TILE - 1) / ENC_TILE;
    const int b0 = min((int)threadIdx.x * per, P.nblocks), b1 = min(b0 + per, P.nblocks);
    uint32_t s = 0;
    for (int b = b0; b < b1; ++b) s += o[b];
    uint32_t total;
    uint32_t at = block_scan(s, sh, total);
    for (int b = b0; b < b1; ++b) {
        const uint32_t l = o[b];
        o[b] = at;
        at += l;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(const JEnc P, const int16_t* __restrict__ coef, const uint32_t* __restrict__ off,
                                                            uint32_t* __restrict__ bits)
{
    __shared__ uint32_t huff[4][256];
    load_huff(huff);
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= P.nblocks) return;
    const int f = blockIdx.y;
    const uint32_t o = off[(size_t)f * P.nblocks + blk];
    uint32_t* w = bits + (size_t)f * P.words_cap + (o >> 5);
    uint64_t acc = 0;
    int cnt = o & 31;                              // bits of the word in front that belong to the blocks before
    bool shared = cnt != 0;
    code_block(P, coef + (size_t)f * P.nblocks * 64, blk, huff, [&](uint32_t code, int len) {
        acc |= (uint64_t)code << (64 - cnt - len);
        cnt += len;
        if (cnt >= 32) {
            const uint32_t word = (uint32_t)(acc >> 32);
            if (shared)
                atomicOr(w, word);
            else
                *w = word;
            shared = false;
            ++w;
            acc <<= 32;
            cnt -= 32;
        }
    });
    if (cnt > 0) atomicOr(w, (uint32_t)(acc >> 32));
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// byte stuffing

__device__ __forceinline__ int ff_count(uint32_t word, int valid)   // 0xFF bytes among the first `valid` (big-endian) bytes
{
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (j < valid && ((word >> (24 - 8 * j)) & 255) == 255) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(ENC_TILE) void jpeg_enc_stuff_kernel(const JEnc P, const uint32_t* __restrict__ bits, const uint32_t* __restrict__ totals,
                                                                  uint8_t* __restrict__ out, uint32_t stride, int* __restrict__ lengths,
                                                                  int* __restrict__ status)
{
    __shared__ uint32_t sh[ENC_TILE / 64];
    const int f = blockIdx.x;
    const uint32_t T = totals[f];
    const uint32_t nbytes = (T + 7) >> 3, nwords = (nbytes + 3) >> 2;
    const uint32_t* src = bits + (size_t)f * P.words_cap;
    // the last byte is padded with one-bits
    const uint32_t pad_word = T >> 5;
    uint32_t pad_mask = 0;
    if (T & 7) {
        const int from = T & 31, to = (int)(((T + 7) & ~7u) - (T & ~31u));     // bit positions [from, to) of pad_word, 0 = the top bit
        pad_mask = (uint32_t)((((uint64_t)1 << (32 - from)) - 1) & ~(((uint64_t)1 << (32 - to)) - 1));
    }
    auto word_at = [&](uint32_t i) { return src[i] | (i == pad_word ? pad_mask : 0u); };
    auto valid_at = [&](uint32_t i) { return (int)min(4u, nbytes - 4 * i); };
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < nwords; i += ENC_TILE) c += ff_count(word_at(i), valid_at(i));
    uint32_t nff;
    block_scan(c, sh, nff);
    const uint64_t need = (uint64_t)P.hdr_len + nbytes + nff + 2;
    const bool fits = need <= stride;
    if (threadIdx.x == 0) {
        lengths[f] = (int)min(need, (uint64_t)0x7FFFFFFF);
        status[f] = fits ? 0 : 1;
    }
    if (!fits) return;                             // uniform over the workgroup
    uint8_t* dst = out + (size_t)f * stride;
    for (int i = threadIdx.x; i < P.hdr_len; i += ENC_TILE) dst[i] = P.header[i];
    dst += P.hdr_len;
    uint32_t ff_before = 0;
    for (uint32_t base = 0; base < nwords; base += ENC_TILE) {
        const uint32_t i = base + threadIdx.x;
        uint32_t word = 0;
        int valid = 0;
        if (i < nwords) {
            word = word_at(i);
            valid = valid_at(i);
        }
        uint32_t tile_ff;
        uint32_t at = 4 * i + ff_before + block_scan(ff_count(word, valid), sh, tile_ff);
        for (int j = 0; j < valid; ++j) {
            const uint8_t b = (word >> (24 - 8 * j)) & 255;
            dst[at++] = b;
            if (b == 255) dst[at++] = 0;
        }
        ff_before += tile_ff;
    }
    if (threadIdx.x == 0) {
        dst[nbytes + nff] = 0xFF;
        dst[nbytes + nff + 1] = 0xD9;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// drawing

constexpr int DRAW_REC_INTS = 32;   // 5 rectangles x (x0, y0, x1, y1) inclusive and clipped (x1 < x0: empty); [20] colour, [21] ink (byte k = channel
                                    // k of the frame's memory order); [22..26] mask x, y, w, h, offset into the atlas (w = 0: no label)

__global__ __launch_bounds__(256) void draw_boxes_kernel(uint8_t* __restrict__ frames, int h, int w, long pixels, const int* __restrict__ rec_begin,
                                                         const int* __restrict__ recs, const uint8_t* __restrict__ atlas)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= pixels) return;
    const int f = (int)(t / ((long)h * w));
    const int r = (int)(t % ((long)h * w));
    const int y = r / w, x = r % w;
    const int r0 = rec_begin[f], r1 = rec_begin[f + 1];
    if (r0 == r1) return;
    uint8_t* p = frames + t * 3;
    int c0 = p[0], c1 = p[1], c2 = p[2];
    bool changed = false;
    for (int k = r0; k < r1; ++k) {
        const int* R = recs + (size_t)k * DRAW_REC_INTS;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (x >= R[4 * q] && x <= R[4 * q + 2] && y >= R[4 * q + 1] && y <= R[4 * q + 3]) {
                const int col = R[20];
                c0 = col & 255, c1 = (col >> 8) & 255, c2 = (col >> 16) & 255;
                changed = true;
            }
        }
        const int mx = x - R[22], my = y - R[23];
        if (mx >= 0 && mx < R[24] && my >= 0 && my < R[25]) {
            const int m = atlas[R[26] + my * R[24] + mx];
            const int ink = R[21];
            int tt = c0 * (255 - m) + (ink & 255) * m + 128;
            c0 = ((tt >> 8) + tt) >> 8;
            tt = c1 * (255 - m) + ((ink >> 8) & 255) * m + 128;
            c1 = ((tt >> 8) + tt) >> 8;
            tt = c2 * (255 - m) + ((ink >> 16) & 255) * m + 128;
            c2 = ((tt >> 8) + tt) >> 8;
            changed = true;
        }
    }
    if (changed) p[0] = (uint8_t)c0, p[1] = (uint8_t)c1, p[2] = (uint8_t)c2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host

void put_seg(uint8_t* h, int& n, int marker, const uint8_t* payload, int len)
{
    h[n++] = 0xFF, h[n++] = (uint8_t)marker, h[n++] = (uint8_t)((len + 2) >> 8), h[n++] = (uint8_t)((len + 2) & 255);
    memcpy(h + n, payload, len);
    n += len;
}

const JEnc* enc_of(const void* blob)
{
    const JEnc* P = static_cast<const JEnc*>(blob);
    return P && P->magic == ENC_MAGIC ? P : nullptr;
}

}  // namespace

extern "C" {

int yf_jpeg_enc_setup(int h, int w, int channels, int quality, int subsampling, void* host_blob, size_t blob_cap, size_t* blob_bytes)
{
    if (h < 1 || w < 1 || h > ENC_MAX_DIM || w > ENC_MAX_DIM) return fail(YF_E_INVALID, "yf_jpeg_enc_setup: sides must be 1..%d, got %d x %d", ENC_MAX_DIM, h, w);
    if (channels != 1 && channels != 3) return fail(YF_E_INVALID, "yf_jpeg_enc_setup: 1 (gray) or 3 channels, got %d", channels);
    if (quality < 1 || quality > 100) return fail(YF_E_INVALID, "yf_jpeg_enc_setup: quality must be 1..100, got %d", quality);
    if (subsampling < 0 || subsampling > 2) return fail(YF_E_INVALID, "yf_jpeg_enc_setup: subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), got %d", subsampling);
    JEnc P;
    memset(&P, 0, sizeof P);
    P.magic = ENC_MAGIC;
    P.h = h, P.w = w, P.ncomp = channels, P.quality = quality;
    P.hs = channels == 3 && subsampling >= 1 ? 2 : 1;
    P.vs = channels == 3 && subsampling == 2 ? 2 : 1;
    P.mcu_rows = (h + 8 * P.vs - 1) / (8 * P.vs);
    P.mcu_cols = (w + 8 * P.hs - 1) / (8 * P.hs);
    P.bpm = channels == 3 ? P.hs * P.vs + 2 : 1;
    const long nblocks = (long)P.mcu_rows * P.mcu_cols * P.bpm;
    if (nblocks * ENC_BLOCK_BITS >= (1L << 31))
        return fail(YF_E_INVALID, "yf_jpeg_enc_setup: %d x %d x %d: the worst-case stream exceeds 2^31 bits", h, w, channels);
    P.nblocks = (int)nblocks;
    P.words_cap = (uint32_t)(nblocks * (ENC_BLOCK_BITS / 32) + 2);
    // jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    uint8_t q[2][64];
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            long v = ((long)K_Q[t][k] * scale + 50) / 100;
            v = v < 1 ? 1 : v > 255 ? 255 : v;
            q[t][k] = (uint8_t)v;
            P.div[t][ZIGZAG[k]] = (uint16_t)(8 * v);
            P.rcp[t][ZIGZAG[k]] = (uint32_t)((1ull << 32) / (uint64_t)(8 * v) + 1);
        }
    uint8_t* hd = P.header;
    int n = 0;
    hd[n++] = 0xFF, hd[n++] = 0xD8;
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_seg(hd, n, 0xE0, jfif, 14);
    const int ntab = channels == 3 ? 2 : 1;
    uint8_t seg[200];
    for (int t = 0; t < ntab; ++t) {
        seg[0] = (uint8_t)t;
        memcpy(seg + 1, q[t], 64);
        put_seg(hd, n, 0xDB, seg, 65);
    }
    int m = 0;
    seg[m++] = 8, seg[m++] = (uint8_t)(h >> 8), seg[m++] = (uint8_t)(h & 255), seg[m++] = (uint8_t)(w >> 8), seg[m++] = (uint8_t)(w & 255);
    seg[m++] = (uint8_t)channels;
    for (int c = 0; c < channels; ++c) {
        seg[m++] = (uint8_t)(c + 1);
        seg[m++] = (uint8_t)(c == 0 ? (P.hs << 4 | P.vs) : 0x11);
        seg[m++] = (uint8_t)(c ? 1 : 0);
    }
    put_seg(hd, n, 0xC0, seg, m);
    for (int t = 0; t < ntab; ++t)
        for (int cls = 0; cls < 2; ++cls) {
            const uint8_t* bits = cls ? K_AC_BITS[t] : K_DC_BITS[t];
            const uint8_t* vals = cls ? K_AC_VALS[t] : K_DC_VALS;
            const int nv = cls ? 162 : 12;
            seg[0] = (uint8_t)(cls << 4 | t);
            memcpy(seg + 1, bits, 16);
            memcpy(seg + 17, vals, nv);
            put_seg(hd, n, 0xC4, seg, 17 + nv);
        }
    m = 0;
    seg[m++] = (uint8_t)channels;
    for (int c = 0; c < channels; ++c) seg[m++] = (uint8_t)(c + 1), seg[m++] = (uint8_t)(c ? 0x11 : 0);
    seg[m++] = 0, seg[m++] = 63, seg[m++] = 0;
    put_seg(hd, n, 0xDA, seg, m);
    P.hdr_len = n;
    if (blob_bytes) *blob_bytes = sizeof(JEnc);
    if (!host_blob) return YF_OK;
    if (blob_cap < sizeof(JEnc)) return fail(YF_E_INVALID, "yf_jpeg_enc_setup: blob capacity %zu B < %zu B", blob_cap, sizeof(JEnc));
    memcpy(host_blob, &P, sizeof P);
    return YF_OK;
}

int yf_jpeg_enc_info(const void* host_blob, int* info, int n_info, uint8_t* header, uint16_t* divisors, uint32_t* reciprocals)
{
    const JEnc* P = enc_of(host_blob);
    if (!P) return fail(YF_E_BLOB, "yf_jpeg_enc_info: not a blob of yf_jpeg_enc_setup");
    const int v[10] = {P->h, P->w, P->ncomp, P->hs, P->vs, P->quality, P->hdr_len, P->nblocks, P->bpm, (int)sizeof(JEnc)};
    for (int i = 0; info && i < n_info && i < 10; ++i) info[i] = v[i];
    if (header) memcpy(header, P->header, P->hdr_len);
    if (divisors) memcpy(divisors, P->div, sizeof P->div);
    if (reciprocals) memcpy(reciprocals, P->rcp, sizeof P->rcp);
    return YF_OK;
}

int yf_jpeg_enc_workspace_bytes(const void* host_blob, int n, size_t* bytes)
{
    const JEnc* P = enc_of(host_blob);
    if (!P || !bytes || n < 0) return fail(YF_E_BLOB, "yf_jpeg_enc_workspace_bytes: not a blob of yf_jpeg_enc_setup, or no frames");
    *bytes = enc_ws(*P, n).end;
    return YF_OK;
}

int yf_jpeg_encode_u8(int device, const void* host_blob, const uint8_t* d_frames, int n, int bgr, void* d_workspace, size_t ws_bytes, uint8_t* d_out,
                      size_t stride, int* d_lengths, int* d_status, void* stream)
{
    const JEnc* Pp = enc_of(host_blob);
    if (!Pp || !d_frames || !d_out || !d_lengths || !d_status) return fail(YF_E_INVALID, "yf_jpeg_encode_u8: null pointer or not a blob of yf_jpeg_enc_setup");
    if (n < 1 || n > 65535) return fail(YF_E_INVALID, "yf_jpeg_encode_u8: 1..65535 frames in one call, got %d", n);
    if (stride < 1 || stride > 0x7FFFFFFF) return fail(YF_E_INVALID, "yf_jpeg_encode_u8: stride must be 1..2^31-1 bytes");
    const JEnc P = *Pp;
    const EncWs s = enc_ws(P, n);
    if (!d_workspace || ws_bytes < s.end) return fail(YF_E_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, s.end);
    if ((uintptr_t)d_workspace % 256) return fail(YF_E_INVALID, "yf_jpeg_encode_u8: workspace must be 256-byte aligned");
    HIP_OK(hipSetDevice(device));
    const hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    int16_t* coef = reinterpret_cast<int16_t*>(ws + s.coef);
    uint32_t* off = reinterpret_cast<uint32_t*>(ws + s.off);
    uint32_t* totals = reinterpret_cast<uint32_t*>(ws + s.total);
    uint32_t* bits = reinterpret_cast<uint32_t*>(ws + s.bits);
    HIP_OK(hipMemsetAsync(bits, 0, (size_t)n * P.words_cap * 4, st));
    const dim3 grid((P.nblocks + 255) / 256, n);
    hipLaunchKernelGGL(jpeg_enc_blocks_kernel, grid, dim3(256), 0, st, P, d_frames, bgr ? 1 : 0, coef);
    hipLaunchKernelGGL(jpeg_enc_lengths_kernel, grid, dim3(256), 0, st, P, (const int16_t*)coef, off);
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(n), dim3(ENC_TILE), 0, st, P, off, totals);
    hipLaunchKernelGGL(jpeg_enc_bits_kernel, grid, dim3(256), 0, st, P, (const int16_t*)coef, (const uint32_t*)off, bits);
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(n), dim3(ENC_TILE), 0, st, P, (const uint32_t*)bits, (const uint32_t*)totals, d_out,
                       (uint32_t)stride, d_lengths, d_status);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

int yf_draw_boxes_u8(int device, uint8_t* d_frames, int n, int h, int w, const int* d_rec_begin, const int* d_records, const uint8_t* d_atlas,
                     void* stream)
{
    if (!d_frames || !d_rec_begin || !d_records || !d_atlas) return fail(YF_E_INVALID, "yf_draw_boxes_u8: null pointer");
    if (n < 1 || h < 1 || w < 1) return fail(YF_E_INVALID, "yf_draw_boxes_u8: no frames or an empty frame");
    HIP_OK(hipSetDevice(device));
    const long pixels = (long)n * h * w;
    if ((pixels + 255) / 256 > 0x7FFFFFFFL) return fail(YF_E_INVALID, "yf_draw_boxes_u8: too many pixels for one launch");
    hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_frames, h, w, pixels,
                       d_rec_begin, d_records, d_atlas);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

}  // extern "C"
