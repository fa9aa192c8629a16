// jpeg_core.h -- the three workgroup programs of the JPEG encoder (include/gp_jpeg.h), written as phases exactly as png_core.h is: inside
// PNG_PHASE(t) ... PNG_END every lane t of the workgroup runs the body and a barrier follows; nothing lives in a register across
// phases.  Under hipcc a phase is the lane's own code; without it (tests/jpeg_emulate.cpp) it is a loop over the lanes, so the same
// text encodes on a CPU, byte for byte: all arithmetic is on integers.
#pragma once
#include "../../include/gp_jpeg.h"
#include "png_core.h"

#define JPG_BLOCK PNG_BLOCK
#define JPG_R GP_JPEG_RESTART_MCUS
#define JPG_MAX_BLOCKS (6 * JPG_R)                                   // blocks of one interval (4:2:0)
#define JPG_BSTRIDE 72                                               // words of a block in `work`: rows of 9, so that neither a lane per row
#define JPG_RSTRIDE 9                                                //   (stride 9) nor a lane per column (block stride 72 = 8 mod 32) meets a bank twice
#define JPG_QSTRIDE 66                                               // int16 of a block in `q`: 33 words, odd, for the lane-per-block walks
#define JPG_SEG_BYTES(nblocks) (((nblocks) * GP_JPEG_BLOCK_BITS + 7) / 8)          // an interval before stuffing, at most
#define JPG_BIT_WORDS (JPG_SEG_BYTES(JPG_MAX_BLOCKS) / 4 + 2)        // (+ the word a put may touch)
#define JPG_MAX_STUFFED (2 * JPG_SEG_BYTES(JPG_MAX_BLOCKS))
#define JPG_HEAD GP_JPEG_HEAD_BYTES

#if defined(__HIP_DEVICE_COMPILE__)
#define JPG_TABLE static __device__ const          // (the host pass of hipcc sees plain constants: the header is built on the host)
#else
#define JPG_TABLE static const
#endif

// Annex K.3 tables (BITS, HUFFVAL) as the DHT segments hold them; JPG_DC_CODE / JPG_AC_CODE: the codes they generate, code | length << 16,
// indexed [table][symbol]; the Annex K.1 quantisation tables in natural order; the zigzag scan and its inverse; K = round(C * 2^24).
JPG_TABLE uint8_t JPG_BITS_DC_LUM[16] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
};
JPG_TABLE uint8_t JPG_VALS_DC_LUM[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
JPG_TABLE uint8_t JPG_BITS_AC_LUM[16] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
};
JPG_TABLE uint8_t JPG_VALS_AC_LUM[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
    36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
    74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
    138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
    198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
    249, 250,
};
JPG_TABLE uint8_t JPG_BITS_DC_CHR[16] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
};
JPG_TABLE uint8_t JPG_VALS_DC_CHR[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
JPG_TABLE uint8_t JPG_BITS_AC_CHR[16] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
};
JPG_TABLE uint8_t JPG_VALS_AC_CHR[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
    21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
    73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
    136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195,
    196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248,
    249, 250,
};
JPG_TABLE uint32_t JPG_DC_CODE[24] = {
    131072, 196610, 196611, 196612, 196613, 196614, 262158, 327710, 393278, 458878, 524542, 590334,
    131072, 131073, 131074, 196614, 262158, 327710, 393278, 458878, 524542, 590334, 656382, 722942,
};
JPG_TABLE uint32_t JPG_AC_CODE[512] = {
    262154, 131072, 131073, 196612, 262155, 327706, 458872, 524536, 656374, 1113986, 1113987, 0, 0, 0, 0, 0,
    0, 262156, 327707, 458873, 590326, 722934, 1113988, 1113989, 1113990, 1113991, 1113992, 0, 0, 0, 0, 0,
    0, 327708, 524537, 656375, 790516, 1113993, 1113994, 1113995, 1113996, 1113997, 1113998, 0, 0, 0, 0, 0,
    0, 393274, 590327, 790517, 1113999, 1114000, 1114001, 1114002, 1114003, 1114004, 1114005, 0, 0, 0, 0, 0,
    0, 393275, 656376, 1114006, 1114007, 1114008, 1114009, 1114010, 1114011, 1114012, 1114013, 0, 0, 0, 0, 0,
    0, 458874, 722935, 1114014, 1114015, 1114016, 1114017, 1114018, 1114019, 1114020, 1114021, 0, 0, 0, 0, 0,
    0, 458875, 790518, 1114022, 1114023, 1114024, 1114025, 1114026, 1114027, 1114028, 1114029, 0, 0, 0, 0, 0,
    0, 524538, 790519, 1114030, 1114031, 1114032, 1114033, 1114034, 1114035, 1114036, 1114037, 0, 0, 0, 0, 0,
    0, 590328, 1015744, 1114038, 1114039, 1114040, 1114041, 1114042, 1114043, 1114044, 1114045, 0, 0, 0, 0, 0,
    0, 590329, 1114046, 1114047, 1114048, 1114049, 1114050, 1114051, 1114052, 1114053, 1114054, 0, 0, 0, 0, 0,
    0, 590330, 1114055, 1114056, 1114057, 1114058, 1114059, 1114060, 1114061, 1114062, 1114063, 0, 0, 0, 0, 0,
    0, 656377, 1114064, 1114065, 1114066, 1114067, 1114068, 1114069, 1114070, 1114071, 1114072, 0, 0, 0, 0, 0,
    0, 656378, 1114073, 1114074, 1114075, 1114076, 1114077, 1114078, 1114079, 1114080, 1114081, 0, 0, 0, 0, 0,
    0, 722936, 1114082, 1114083, 1114084, 1114085, 1114086, 1114087, 1114088, 1114089, 1114090, 0, 0, 0, 0, 0,
    0, 1114091, 1114092, 1114093, 1114094, 1114095, 1114096, 1114097, 1114098, 1114099, 1114100, 0, 0, 0, 0, 0,
    722937, 1114101, 1114102, 1114103, 1114104, 1114105, 1114106, 1114107, 1114108, 1114109, 1114110, 0, 0, 0, 0, 0,
    131072, 131073, 196612, 262154, 327704, 327705, 393272, 458872, 590324, 656374, 790516, 0, 0, 0, 0, 0,
    0, 262155, 393273, 524534, 590325, 722934, 790517, 1113992, 1113993, 1113994, 1113995, 0, 0, 0, 0, 0,
    0, 327706, 524535, 656375, 790518, 1015746, 1113996, 1113997, 1113998, 1113999, 1114000, 0, 0, 0, 0, 0,
    0, 327707, 524536, 656376, 790519, 1114001, 1114002, 1114003, 1114004, 1114005, 1114006, 0, 0, 0, 0, 0,
    0, 393274, 590326, 1114007, 1114008, 1114009, 1114010, 1114011, 1114012, 1114013, 1114014, 0, 0, 0, 0, 0,
    0, 393275, 656377, 1114015, 1114016, 1114017, 1114018, 1114019, 1114020, 1114021, 1114022, 0, 0, 0, 0, 0,
    0, 458873, 722935, 1114023, 1114024, 1114025, 1114026, 1114027, 1114028, 1114029, 1114030, 0, 0, 0, 0, 0,
    0, 458874, 722936, 1114031, 1114032, 1114033, 1114034, 1114035, 1114036, 1114037, 1114038, 0, 0, 0, 0, 0,
    0, 524537, 1114039, 1114040, 1114041, 1114042, 1114043, 1114044, 1114045, 1114046, 1114047, 0, 0, 0, 0, 0,
    0, 590327, 1114048, 1114049, 1114050, 1114051, 1114052, 1114053, 1114054, 1114055, 1114056, 0, 0, 0, 0, 0,
    0, 590328, 1114057, 1114058, 1114059, 1114060, 1114061, 1114062, 1114063, 1114064, 1114065, 0, 0, 0, 0, 0,
    0, 590329, 1114066, 1114067, 1114068, 1114069, 1114070, 1114071, 1114072, 1114073, 1114074, 0, 0, 0, 0, 0,
    0, 590330, 1114075, 1114076, 1114077, 1114078, 1114079, 1114080, 1114081, 1114082, 1114083, 0, 0, 0, 0, 0,
    0, 722937, 1114084, 1114085, 1114086, 1114087, 1114088, 1114089, 1114090, 1114091, 1114092, 0, 0, 0, 0, 0,
    0, 933856, 1114093, 1114094, 1114095, 1114096, 1114097, 1114098, 1114099, 1114100, 1114101, 0, 0, 0, 0, 0,
    656378, 1015747, 1114102, 1114103, 1114104, 1114105, 1114106, 1114107, 1114108, 1114109, 1114110, 0, 0, 0, 0, 0,
};
JPG_TABLE uint8_t JPG_BASE_LUM[64] = {
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99,
};
JPG_TABLE uint8_t JPG_BASE_CHR[64] = {
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
};
JPG_TABLE uint8_t JPG_ZIGZAG[64] = {
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
};
JPG_TABLE uint8_t JPG_ZIGZAG_OF[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};
JPG_TABLE int32_t JPG_DCT[64] = {
    5931642, 5931642, 5931642, 5931642, 5931642, 5931642, 5931642, 5931642,
    8227423, 6974873, 4660461, 1636536, -1636536, -4660461, -6974873, -8227423,
    7750063, 3210181, -3210181, -7750063, -7750063, -3210181, 3210181, 7750063,
    6974873, -1636536, -8227423, -4660461, 4660461, 8227423, 1636536, -6974873,
    5931642, -5931642, -5931642, 5931642, 5931642, -5931642, -5931642, 5931642,
    4660461, -8227423, 1636536, 6974873, -6974873, -1636536, 8227423, -4660461,
    3210181, -7750063, 7750063, -3210181, -3210181, 7750063, -7750063, 3210181,
    1636536, -4660461, 6974873, -8227423, 8227423, -6974873, 4660461, -1636536,
};

struct JpgPlan {
    int B, H, W;
    int sub;                 // GP_JPEG_420 / GP_JPEG_444
    int msize;               // pixels of an MCU's side: 16 / 8
    int mblocks;             // blocks of an MCU: 6 / 3
    int mw, mh;              // MCUs per row, MCU rows
    int nmcu, nseg;
    int src_kind;
    const void* src;
    uint8_t* seg;            // [B][nseg][seg_stride]: the stuffed intervals
    uint32_t seg_stride;
    uint32_t* seg_len;       // [B][nseg]
    uint32_t* seg_off;       // [B][nseg]: where the interval starts in the file
    uint8_t* out;
    int64_t out_stride;
    uint32_t* sizes;
    uint8_t qt[2][64];       // natural order
    uint8_t head[JPG_HEAD + 3];
};

// ---- host: tables, sizes, the header ---------------------------------------------------------------------------------------------
static inline void jpg_quant_tables(int quality, uint8_t* lum, uint8_t* chr) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (JPG_BASE_LUM[i] * scale + 50) / 100, c = (JPG_BASE_CHR[i] * scale + 50) / 100;
        lum[i] = (uint8_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chr[i] = (uint8_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
}

static inline void jpg_plan_sizes(JpgPlan& p, int B, int H, int W, int sub) {
    p.B = B; p.H = H; p.W = W; p.sub = sub;
    p.msize = sub == GP_JPEG_420 ? 16 : 8;
    p.mblocks = sub == GP_JPEG_420 ? 6 : 3;
    p.mw = (W + p.msize - 1) / p.msize;
    p.mh = (H + p.msize - 1) / p.msize;
    p.nmcu = p.mw * p.mh;
    p.nseg = (p.nmcu + JPG_R - 1) / JPG_R;
    p.seg_stride = (uint32_t)((2 * JPG_SEG_BYTES(JPG_R * p.mblocks) + 15) / 16 * 16);
}

// every interval at its largest and stuffed, the two bytes behind each, the header; a multiple of 8
static inline int64_t jpg_bound_of(const JpgPlan& p) {
    const int64_t last = p.nmcu - (int64_t)(p.nseg - 1) * JPG_R;
    return (JPG_HEAD + (int64_t)(p.nseg - 1) * (2 * JPG_SEG_BYTES(JPG_R * p.mblocks) + 2) + 2 * JPG_SEG_BYTES(last * p.mblocks) + 2 + 7) / 8 * 8;
}

static inline int jpg_dht(uint8_t* d, int tc_th, const uint8_t* bits, const uint8_t* vals, int nvals) {
    int n = 0;
    d[n++] = 0xff; d[n++] = 0xc4; d[n++] = 0; d[n++] = (uint8_t)(19 + nvals); d[n++] = (uint8_t)tc_th;
    for (int i = 0; i < 16; ++i) d[n++] = bits[i];
    for (int i = 0; i < nvals; ++i) d[n++] = vals[i];
    return n;
}

// SOI .. SOS into p.head, from p.H, p.W, p.sub and p.qt
static inline int jpg_build_header(JpgPlan& p) {
    uint8_t* d = p.head;
    int n = 0;
    const uint8_t app0[20] = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; ++i) d[n++] = app0[i];
    for (int t = 0; t < 2; ++t) {
        d[n++] = 0xff; d[n++] = 0xdb; d[n++] = 0; d[n++] = 67; d[n++] = (uint8_t)t;
        for (int k = 0; k < 64; ++k) d[n++] = p.qt[t][JPG_ZIGZAG[k]];
    }
    const uint8_t s0 = p.sub == GP_JPEG_420 ? 0x22 : 0x11;
    const uint8_t sof[19] = {0xff, 0xc0, 0, 17, 8, (uint8_t)(p.H >> 8), (uint8_t)p.H, (uint8_t)(p.W >> 8), (uint8_t)p.W, 3, 1, s0, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (int i = 0; i < 19; ++i) d[n++] = sof[i];
    n += jpg_dht(d + n, 0x00, JPG_BITS_DC_LUM, JPG_VALS_DC_LUM, 12);
    n += jpg_dht(d + n, 0x10, JPG_BITS_AC_LUM, JPG_VALS_AC_LUM, 162);
    n += jpg_dht(d + n, 0x01, JPG_BITS_DC_CHR, JPG_VALS_DC_CHR, 12);
    n += jpg_dht(d + n, 0x11, JPG_BITS_AC_CHR, JPG_VALS_AC_CHR, 162);
    const uint8_t tail[20] = {0xff, 0xdd, 0, 4, (uint8_t)(JPG_R >> 8), (uint8_t)(JPG_R & 255), 0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int i = 0; i < 20; ++i) d[n++] = tail[i];
    return n;                                                         // == JPG_HEAD
}

// ---- 1. one restart interval: one workgroup --------------------------------------------------------------------------------------
struct JpgSegShared {
    uint32_t bits[JPG_BIT_WORDS];                  // the interval's bits, MSB first: bit position p is bit 31 - p % 32 of word p / 32
    uint32_t stuffed[JPG_MAX_STUFFED / 4];         // its bytes after stuffing
    int32_t work[JPG_MAX_BLOCKS * JPG_BSTRIDE];    // samples, then the row transform
    int16_t q[JPG_MAX_BLOCKS * JPG_QSTRIDE];       // quantised coefficients in zigzag order
    uint32_t ac[2][256], dc[2][12];                // code | length << 16
    uint32_t blk_bits[JPG_MAX_BLOCKS], blk_off[JPG_MAX_BLOCKS];
    uint32_t lane_ff[JPG_BLOCK], lane_dst[JPG_BLOCK];
    uint32_t nbytes, nstuffed;
};

PNG_FN int jpg_clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// the 8-bit pixel (y, x) of image b, the last row and column replicated beyond the image, as Y Cb Cr
PNG_FN void jpg_ycc(const JpgPlan& p, int b, int y, int x, int& Y, int& Cb, int& Cr) {
    y = y < p.H ? y : p.H - 1;
    x = x < p.W ? x : p.W - 1;
    const size_t plane = (size_t)p.H * p.W, i = (size_t)b * 3 * plane + (size_t)y * p.W + x;
    const int R = png_q8_at(p.src, p.src_kind, i), G = png_q8_at(p.src, p.src_kind, i + plane), B = png_q8_at(p.src, p.src_kind, i + 2 * plane);
    Y = jpg_clamp8((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
    Cb = jpg_clamp8((-11058 * R - 21710 * G + 32768 * B + (128 << 16) + 32768) >> 16);
    Cr = jpg_clamp8((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32768) >> 16);
}

PNG_FN int jpg_category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}
PNG_FN uint32_t jpg_extra(int v, int cat) { return (uint32_t)(v >= 0 ? v : v + (1 << cat) - 1); }

// the component (0 luminance, 1 chrominance table) of block k of an MCU, and the block that holds its DC predictor (-1: none)
PNG_FN int jpg_block_table(const JpgPlan& p, int k) { return p.sub == GP_JPEG_420 ? (k >= 4) : (k >= 1); }
PNG_FN int jpg_block_before(const JpgPlan& p, int blk) {
    const int m = blk / p.mblocks, k = blk - m * p.mblocks;
    if (p.sub == GP_JPEG_420 && k >= 1 && k < 4) return blk - 1;
    if (m == 0) return -1;
    return blk - p.mblocks + ((p.sub == GP_JPEG_420 && k == 0) ? 3 : 0);
}

// the codes of one block: f.put(value, nbits) with nbits <= 26
template <class F>
PNG_FN void jpg_walk(const int16_t* q, int pred, const uint32_t* dc, const uint32_t* ac, F& f) {
    const int diff = q[0] - pred, dcat = jpg_category(diff);
    f.put(((dc[dcat] & 0xffffu) << dcat) | jpg_extra(diff, dcat), (int)(dc[dcat] >> 16) + dcat);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = q[k];
        if (v == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) f.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
        const int cat = jpg_category(v);
        const uint32_t e = ac[(run << 4) | cat];
        f.put(((e & 0xffffu) << cat) | jpg_extra(v, cat), (int)(e >> 16) + cat);
        run = 0;
    }
    if (run) f.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

struct JpgMeasure {
    uint32_t n;
    PNG_MEMBER void put(uint32_t, int nbits) { n += (uint32_t)nbits; }
};

PNG_FN void jpg_put(uint32_t* out, uint32_t pos, uint32_t value, int nbits) {          // 1 <= nbits <= 32, value < 2^nbits
    const uint32_t w = pos >> 5;
    const int end = (int)(pos & 31) + nbits;
    if (end <= 32) {
        PNG_OR(&out[w], value << (32 - end));
    } else {
        PNG_OR(&out[w], value >> (end - 32));
        PNG_OR(&out[w + 1], value << (64 - end));
    }
}

struct JpgEmit {
    uint32_t* out;
    uint32_t pos;
    PNG_MEMBER void put(uint32_t value, int nbits) { jpg_put(out, pos, value, nbits); pos += (uint32_t)nbits; }
};

PNG_FN uint32_t jpg_byte(const uint32_t* bits, uint32_t i) { return (bits[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

PNG_FN void jpg_segment_block(JpgSegShared& sh, const JpgPlan& p, int b, int s) {
    const int m0 = s * JPG_R, nm = p.nmcu - m0 < JPG_R ? p.nmcu - m0 : JPG_R, nblk = nm * p.mblocks;
    const int nwords = JPG_SEG_BYTES(nblk) / 4 + 2;
    PNG_PHASE(t)
        for (int w = t; w < nwords; w += JPG_BLOCK) sh.bits[w] = 0;
        for (int i = t; i < 512; i += JPG_BLOCK) sh.ac[i >> 8][i & 255] = JPG_AC_CODE[i];
        if (t < 24) sh.dc[t / 12][t % 12] = JPG_DC_CODE[t];
        // a unit is one pixel (4:4:4) or 2 x 2 pixels (4:2:0), 64 to an MCU; units in the order (row of the MCU, MCU, column), so that
        // neighbouring lanes read neighbouring pixels across the interval's MCUs
        for (int u = t; u < nm * 64; u += JPG_BLOCK) {
            const int uy = u / (nm * 8), m = (u >> 3) % nm, ux = u & 7;
            const int my = (m0 + m) / p.mw, mx = (m0 + m) - my * p.mw;
            int32_t* blocks = sh.work + m * p.mblocks * JPG_BSTRIDE;
            if (p.sub == GP_JPEG_420) {
                int cb = 2, cr = 2;
                for (int dy = 0; dy < 2; ++dy)
                    for (int dx = 0; dx < 2; ++dx) {
                        const int py = 2 * uy + dy, px = 2 * ux + dx;
                        int Y, Cb, Cr;
                        jpg_ycc(p, b, my * 16 + py, mx * 16 + px, Y, Cb, Cr);
                        blocks[((py >> 3) * 2 + (px >> 3)) * JPG_BSTRIDE + (py & 7) * JPG_RSTRIDE + (px & 7)] = Y - 128;
                        cb += Cb;
                        cr += Cr;
                    }
                blocks[4 * JPG_BSTRIDE + uy * JPG_RSTRIDE + ux] = (cb >> 2) - 128;
                blocks[5 * JPG_BSTRIDE + uy * JPG_RSTRIDE + ux] = (cr >> 2) - 128;
            } else {
                int Y, Cb, Cr;
                jpg_ycc(p, b, my * 8 + uy, mx * 8 + ux, Y, Cb, Cr);
                blocks[uy * JPG_RSTRIDE + ux] = Y - 128;
                blocks[JPG_BSTRIDE + uy * JPG_RSTRIDE + ux] = Cb - 128;
                blocks[2 * JPG_BSTRIDE + uy * JPG_RSTRIDE + ux] = Cr - 128;
            }
        }
    PNG_END
    PNG_PHASE(t)                                                      // rows: a lane per row of a block, in place
        for (int l = t; l < nblk * 8; l += JPG_BLOCK) {
            int32_t* row = sh.work + (l >> 3) * JPG_BSTRIDE + (l & 7) * JPG_RSTRIDE;
            int32_t v[8];
            for (int x = 0; x < 8; ++x) v[x] = row[x];
            for (int u = 0; u < 8; ++u) {
                int64_t a = 4;
                for (int x = 0; x < 8; ++x) a += (int64_t)JPG_DCT[u * 8 + x] * v[x];
                row[u] = (int32_t)(a >> 3);
            }
        }
    PNG_END
    PNG_PHASE(t)                                                      // columns and the quantisation: a lane per column of a block
        for (int l = t; l < nblk * 8; l += JPG_BLOCK) {
            const int blk = l >> 3, u = l & 7;
            const uint8_t* qt = p.qt[jpg_block_table(p, blk % p.mblocks)];
            const int32_t* col = sh.work + blk * JPG_BSTRIDE + u;
            int32_t r[8];
            for (int y = 0; y < 8; ++y) r[y] = col[y * JPG_RSTRIDE];
            for (int v = 0; v < 8; ++v) {
                int64_t a = (int64_t)1 << 28;
                for (int y = 0; y < 8; ++y) a += (int64_t)JPG_DCT[v * 8 + y] * r[y];
                const int32_t f16 = (int32_t)(a >> 29);
                const uint32_t qv = qt[v * 8 + u];
                uint32_t n = ((uint32_t)(f16 < 0 ? -f16 : f16) + (qv << 15)) / (qv << 16);
                if ((v | u) && n > 1023u) n = 1023u;
                sh.q[blk * JPG_QSTRIDE + JPG_ZIGZAG_OF[v * 8 + u]] = (int16_t)(f16 < 0 ? -(int32_t)n : (int32_t)n);
            }
        }
    PNG_END
    PNG_PHASE(t)                                                      // a lane per block counts its bits
        if (t < nblk) {
            const int before = jpg_block_before(p, t), tab = jpg_block_table(p, t % p.mblocks);
            JpgMeasure f{0};
            jpg_walk(sh.q + t * JPG_QSTRIDE, before < 0 ? 0 : sh.q[before * JPG_QSTRIDE], sh.dc[tab], sh.ac[tab], f);
            sh.blk_bits[t] = f.n;
        }
    PNG_END
    PNG_PHASE(t)
        if (t < nblk) {
            uint32_t off = 0;
            for (int o = 0; o < t; ++o) off += sh.blk_bits[o];
            sh.blk_off[t] = off;
            if (t == nblk - 1) sh.nbytes = (off + sh.blk_bits[t] + 7) / 8;
        }
    PNG_END
    PNG_PHASE(t)
        if (t < nblk) {
            const int before = jpg_block_before(p, t), tab = jpg_block_table(p, t % p.mblocks);
            JpgEmit f{sh.bits, sh.blk_off[t]};
            jpg_walk(sh.q + t * JPG_QSTRIDE, before < 0 ? 0 : sh.q[before * JPG_QSTRIDE], sh.dc[tab], sh.ac[tab], f);
            if (t == nblk - 1 && (f.pos & 7)) jpg_put(sh.bits, f.pos, (1u << (8 - (f.pos & 7))) - 1, 8 - (int)(f.pos & 7));      // one-bits to the byte's end
        }
    PNG_END
    PNG_PHASE(t)                                                      // stuffing: every lane a slice of the bytes
        const uint32_t per = (sh.nbytes + JPG_BLOCK - 1) / JPG_BLOCK;
        const uint32_t i0 = (uint32_t)t * per < sh.nbytes ? (uint32_t)t * per : sh.nbytes, i1 = i0 + per < sh.nbytes ? i0 + per : sh.nbytes;
        uint32_t ff = 0;
        for (uint32_t i = i0; i < i1; ++i) ff += jpg_byte(sh.bits, i) == 255u;
        sh.lane_ff[t] = ff;
    PNG_END
    PNG_PHASE(t)
        const uint32_t per = (sh.nbytes + JPG_BLOCK - 1) / JPG_BLOCK;
        const uint32_t i0 = (uint32_t)t * per < sh.nbytes ? (uint32_t)t * per : sh.nbytes;
        uint32_t ff = 0;
        for (int o = 0; o < t; ++o) ff += sh.lane_ff[o];
        sh.lane_dst[t] = i0 + ff;
        if (t == JPG_BLOCK - 1) sh.nstuffed = sh.nbytes + ff + sh.lane_ff[t];
    PNG_END
    PNG_PHASE(t)
        const uint32_t per = (sh.nbytes + JPG_BLOCK - 1) / JPG_BLOCK;
        const uint32_t i0 = (uint32_t)t * per < sh.nbytes ? (uint32_t)t * per : sh.nbytes, i1 = i0 + per < sh.nbytes ? i0 + per : sh.nbytes;
        uint8_t* dst = (uint8_t*)sh.stuffed + sh.lane_dst[t];
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t v = jpg_byte(sh.bits, i);
            *dst++ = (uint8_t)v;
            if (v == 255u) *dst++ = 0;
        }
    PNG_END
    PNG_PHASE(t)
        uint32_t* dst32 = (uint32_t*)(p.seg + ((size_t)b * p.nseg + s) * p.seg_stride);     // (seg_stride is a multiple of 16)
        for (uint32_t w = t; w < (sh.nstuffed + 3) / 4; w += JPG_BLOCK) dst32[w] = sh.stuffed[w];
        if (t == 0) p.seg_len[(size_t)b * p.nseg + s] = sh.nstuffed;
    PNG_END
}

// ---- 2. where every interval goes and the file's length: one workgroup per image ------------------------------------------------
struct JpgLayoutShared {
    uint32_t bytes[JPG_BLOCK], start[JPG_BLOCK];
};

PNG_FN void jpg_layout_block(JpgLayoutShared& sh, const JpgPlan& p, int b) {
    const uint32_t* len = p.seg_len + (size_t)b * p.nseg;
    const int per = (p.nseg + JPG_BLOCK - 1) / JPG_BLOCK;
    PNG_PHASE(t)
        const int k0 = t * per < p.nseg ? t * per : p.nseg, k1 = k0 + per < p.nseg ? k0 + per : p.nseg;
        uint32_t bytes = 0;
        for (int k = k0; k < k1; ++k) bytes += len[k] + 2;           // (the interval and the marker behind it: RST or EOI)
        sh.bytes[t] = bytes;
    PNG_END
    PNG_PHASE(t)
        if (t == 0) {
            uint32_t off = JPG_HEAD;
            for (int u = 0; u < JPG_BLOCK; ++u) {
                sh.start[u] = off;
                off += sh.bytes[u];
            }
            p.sizes[b] = off;
        }
    PNG_END
    PNG_PHASE(t)
        const int k0 = t * per < p.nseg ? t * per : p.nseg, k1 = k0 + per < p.nseg ? k0 + per : p.nseg;
        uint32_t off = sh.start[t];
        for (int k = k0; k < k1; ++k) {
            p.seg_off[(size_t)b * p.nseg + k] = off;
            off += len[k] + 2;
        }
    PNG_END
}

// ---- 3. the intervals in place, with the header, the RST markers and EOI: one workgroup per interval ---------------------------
PNG_FN void jpg_copy_block(const JpgPlan& p, int b, int s) {
    const uint32_t len = p.seg_len[(size_t)b * p.nseg + s];
    const uint8_t* src = p.seg + ((size_t)b * p.nseg + s) * p.seg_stride;
    uint8_t* file = p.out + (size_t)b * p.out_stride;
    uint8_t* dst = file + p.seg_off[(size_t)b * p.nseg + s];
    PNG_PHASE(t)
        for (uint32_t i = t; i < len; i += JPG_BLOCK) dst[i] = src[i];
        if (t == 0) {
            dst[len] = 0xff;
            dst[len + 1] = (uint8_t)(s == p.nseg - 1 ? 0xd9 : 0xd0 + (s & 7));
        }
        if (s == 0)
            for (int i = t; i < JPG_HEAD; i += JPG_BLOCK) file[i] = p.head[i];
    PNG_END
}
