/*
 * rt_image.hip -- implementation of include/rt_capi_image.h: a frame's fp32 colours, columns of z, into 8-bit scanlines.  The
 * header is the definition; the kernel is bit-exact to it (the library's arithmetic flags: denormals kept, no fast math).
 *
 * SHAPE.  One memory-shaped pass.  A workgroup owns a tile of kTileX columns by kTileZ pixels.  It reads the
 * tile along z, the input's contiguous axis -- a tile column is 3 kTileZ floats, 384 bytes, three cache lines -- one pixel a
 * lane; quantises at once, so that what goes through LDS is one dword {r, g, b, 255} a pixel and not three floats; and writes
 * the tile along x, the output's contiguous axis: a tile row is C kTileX bytes, 384 or 512.  The LDS image is [x][z] with a pitch
 * of kTileZ + 1 dwords: the z-major writes of a half-wave fall on consecutive banks, the x-major reads on banks x + z.  A code is
 * found by eight comparisons against the 255 thresholds, which travel in the kernel's arguments in the order of an implicit
 * search tree (node i's children 2i and 2i + 1): the nodes of a level are consecutive in LDS, so the first six steps of a wave
 * cannot conflict and equal addresses broadcast.  Every pixel number and byte offset is 64-bit.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rt_capi.h"
#include "../../include/rt_capi_image.h"
#include "rt_host.h"

static_assert(sizeof(rt_image_params) == 24, "rt_image_params layout");
static_assert(offsetof(rt_image_params, exposure) == 12 && offsetof(rt_image_params, thresholds) == 16, "rt_image_params layout");

/* T[1..255] as the nodes of the search tree: e[i], i = 1..255, is T[(2j + 1) << (8 - L)] for node j of level L, i = 2^(L-1) + j
 * (a kernel argument: outside the unnamed namespace, so that the kernel has a name outside this file) */
struct rt_image_search_tree {
    float e[256];
};
using SearchTree = rt_image_search_tree;

namespace {

constexpr int kTileZ = 32, kTileX = 128;               /* a tile: 4096 pixels, 8 a thread */
constexpr int kThreads = 512;
constexpr int kPitch = kTileZ + 1;                     /* dwords between two columns of the LDS image */
constexpr int kPerThread = kTileZ * kTileX / kThreads;
constexpr uint32_t kMaxBlocks = 1u << 22;              /* a workgroup walks the tiles blockIdx.x, + gridDim.x, ... */
constexpr double kMaxStripFloats = 2.0e9 * 4.0;        /* rt_render's limit */
constexpr double kMaxOutBytes = 3.2e10;

/* RT_TRANSFER_SRGB: (float)E((k - 0.5) / 255), k = 1..255 -- these literals are the definition (tests/golden/image/) */
const float kSrgb[255] = {
    0x1.3e4568p-13f, 0x1.dd681cp-12f, 0x1.8dd6c2p-11f, 0x1.167cbap-10f, 0x1.660e14p-10f, 0x1.b59f6ep-10f, 0x1.029864p-9f, 0x1.2a6112p-9f,
    0x1.5229bep-9f, 0x1.79f26ap-9f, 0x1.a1e5a0p-9f, 0x1.cbf734p-9f, 0x1.f86806p-9f, 0x1.13a0bep-8f, 0x1.2c4666p-8f, 0x1.46297ap-8f,
    0x1.614e60p-8f, 0x1.7db96cp-8f, 0x1.9b6edap-8f, 0x1.ba72cep-8f, 0x1.dac95ep-8f, 0x1.fc768ap-8f, 0x1.0fbf22p-7f, 0x1.21f234p-7f,
    0x1.34d662p-7f, 0x1.486d8ep-7f, 0x1.5cb98ep-7f, 0x1.71bc32p-7f, 0x1.877748p-7f, 0x1.9dec90p-7f, 0x1.b51dc8p-7f, 0x1.cd0ca8p-7f,
    0x1.e5bae0p-7f, 0x1.ff2a1ep-7f, 0x1.0cae04p-6f, 0x1.1a291cp-6f, 0x1.28072ap-6f, 0x1.3648f6p-6f, 0x1.44ef4cp-6f, 0x1.53faeep-6f,
    0x1.636ca4p-6f, 0x1.734530p-6f, 0x1.838550p-6f, 0x1.942dc4p-6f, 0x1.a53f48p-6f, 0x1.b6ba94p-6f, 0x1.c8a062p-6f, 0x1.daf168p-6f,
    0x1.edae5cp-6f, 0x1.006bf6p-5f, 0x1.0a3768p-5f, 0x1.1439d8p-5f, 0x1.1e73a0p-5f, 0x1.28e514p-5f, 0x1.338e8ap-5f, 0x1.3e7056p-5f,
    0x1.498acep-5f, 0x1.54de42p-5f, 0x1.606b08p-5f, 0x1.6c316ep-5f, 0x1.7831c6p-5f, 0x1.846c62p-5f, 0x1.90e192p-5f, 0x1.9d91a4p-5f,
    0x1.aa7ce4p-5f, 0x1.b7a3a4p-5f, 0x1.c50630p-5f, 0x1.d2a4d4p-5f, 0x1.e07fdcp-5f, 0x1.ee9794p-5f, 0x1.fcec46p-5f, 0x1.05bf20p-4f,
    0x1.0d26e4p-4f, 0x1.14ad94p-4f, 0x1.1c5356p-4f, 0x1.24184cp-4f, 0x1.2bfc9cp-4f, 0x1.34006ap-4f, 0x1.3c23d6p-4f, 0x1.446708p-4f,
    0x1.4cca1ep-4f, 0x1.554d40p-4f, 0x1.5df08ep-4f, 0x1.66b428p-4f, 0x1.6f9836p-4f, 0x1.789cd4p-4f, 0x1.81c228p-4f, 0x1.8b0850p-4f,
    0x1.946f72p-4f, 0x1.9df7aap-4f, 0x1.a7a11cp-4f, 0x1.b16beap-4f, 0x1.bb5830p-4f, 0x1.c56612p-4f, 0x1.cf95b0p-4f, 0x1.d9e72ap-4f,
    0x1.e45a9ep-4f, 0x1.eef02ep-4f, 0x1.f9a7f8p-4f, 0x1.02410ep-3f, 0x1.07bf5cp-3f, 0x1.0d4ef6p-3f, 0x1.12efecp-3f, 0x1.18a24cp-3f,
    0x1.1e6626p-3f, 0x1.243b8ap-3f, 0x1.2a2286p-3f, 0x1.301b2ap-3f, 0x1.362582p-3f, 0x1.3c41a2p-3f, 0x1.426f94p-3f, 0x1.48af6ap-3f,
    0x1.4f0132p-3f, 0x1.5564f8p-3f, 0x1.5bdacep-3f, 0x1.6262c0p-3f, 0x1.68fce0p-3f, 0x1.6fa938p-3f, 0x1.7667d8p-3f, 0x1.7d38cep-3f,
    0x1.841c28p-3f, 0x1.8b11f6p-3f, 0x1.921a42p-3f, 0x1.99351ep-3f, 0x1.a06296p-3f, 0x1.a7a2bap-3f, 0x1.aef594p-3f, 0x1.b65b34p-3f,
    0x1.bdd3a6p-3f, 0x1.c55efap-3f, 0x1.ccfd3ep-3f, 0x1.d4ae7cp-3f, 0x1.dc72c2p-3f, 0x1.e44a20p-3f, 0x1.ec34a4p-3f, 0x1.f43256p-3f,
    0x1.fc4348p-3f, 0x1.0233c2p-2f, 0x1.064f8ep-2f, 0x1.0a750cp-2f, 0x1.0ea442p-2f, 0x1.12dd3ap-2f, 0x1.171ff8p-2f, 0x1.1b6c82p-2f,
    0x1.1fc2dep-2f, 0x1.242316p-2f, 0x1.288d2cp-2f, 0x1.2d0128p-2f, 0x1.317f12p-2f, 0x1.3606eep-2f, 0x1.3a98c2p-2f, 0x1.3f3496p-2f,
    0x1.43da70p-2f, 0x1.488a54p-2f, 0x1.4d444cp-2f, 0x1.52085ap-2f, 0x1.56d688p-2f, 0x1.5baed8p-2f, 0x1.609154p-2f, 0x1.657e00p-2f,
    0x1.6a74e2p-2f, 0x1.6f7600p-2f, 0x1.748160p-2f, 0x1.79970ap-2f, 0x1.7eb700p-2f, 0x1.83e14cp-2f, 0x1.8915f2p-2f, 0x1.8e54f8p-2f,
    0x1.939e64p-2f, 0x1.98f23ap-2f, 0x1.9e5084p-2f, 0x1.a3b944p-2f, 0x1.a92c80p-2f, 0x1.aeaa42p-2f, 0x1.b4328ap-2f, 0x1.b9c562p-2f,
    0x1.bf62cep-2f, 0x1.c50ad4p-2f, 0x1.cabd7ap-2f, 0x1.d07ac4p-2f, 0x1.d642bap-2f, 0x1.dc1560p-2f, 0x1.e1f2bcp-2f, 0x1.e7dad4p-2f,
    0x1.edcdaep-2f, 0x1.f3cb4ep-2f, 0x1.f9d3bcp-2f, 0x1.ffe6fap-2f, 0x1.030288p-1f, 0x1.061702p-1f, 0x1.0930eep-1f, 0x1.0c504cp-1f,
    0x1.0f7522p-1f, 0x1.129f72p-1f, 0x1.15cf3ep-1f, 0x1.190488p-1f, 0x1.1c3f54p-1f, 0x1.1f7fa4p-1f, 0x1.22c57ap-1f, 0x1.2610dap-1f,
    0x1.2961c8p-1f, 0x1.2cb844p-1f, 0x1.301450p-1f, 0x1.3375f2p-1f, 0x1.36dd2ap-1f, 0x1.3a49fcp-1f, 0x1.3dbc6ap-1f, 0x1.413476p-1f,
    0x1.44b224p-1f, 0x1.483576p-1f, 0x1.4bbe6ep-1f, 0x1.4f4d10p-1f, 0x1.52e15ep-1f, 0x1.567b58p-1f, 0x1.5a1b04p-1f, 0x1.5dc064p-1f,
    0x1.616b7ap-1f, 0x1.651c46p-1f, 0x1.68d2d0p-1f, 0x1.6c8f16p-1f, 0x1.70511cp-1f, 0x1.7418e6p-1f, 0x1.77e672p-1f, 0x1.7bb9c8p-1f,
    0x1.7f92e8p-1f, 0x1.8371d4p-1f, 0x1.875690p-1f, 0x1.8b411cp-1f, 0x1.8f317cp-1f, 0x1.9327b4p-1f, 0x1.9723c4p-1f, 0x1.9b25b0p-1f,
    0x1.9f2d7ap-1f, 0x1.a33b22p-1f, 0x1.a74eb0p-1f, 0x1.ab6820p-1f, 0x1.af877ap-1f, 0x1.b3acbep-1f, 0x1.b7d7ecp-1f, 0x1.bc090cp-1f,
    0x1.c0401ap-1f, 0x1.c47d1ep-1f, 0x1.c8c018p-1f, 0x1.cd090ap-1f, 0x1.d157f6p-1f, 0x1.d5ace0p-1f, 0x1.da07c8p-1f, 0x1.de68b4p-1f,
    0x1.e2cfa2p-1f, 0x1.e73c98p-1f, 0x1.ebaf98p-1f, 0x1.f028a2p-1f, 0x1.f4a7bap-1f, 0x1.f92ce2p-1f, 0x1.fdb81cp-1f
};

} // namespace

/* the number of k in 1..255 with v >= T[k]: T is non-decreasing, so the answers are true up to the code and false after it, and
 * eight steps down the tree count them; a NaN answers false eight times */
__device__ __forceinline__ uint32_t code_of(const float *tree, float v) {
    uint32_t at = 4;                                    /* the node's byte offset: the address needs no shift */
#pragma unroll
    for (int step = 0; step < 8; ++step)
        at = 2u * at + (v >= *reinterpret_cast<const float *>(reinterpret_cast<const char *>(tree) + at) ? 4u : 0u);
    return (at >> 2) - 256u;
}

template <int kC>
__global__ __launch_bounds__(kThreads) void rt_encode_image_kernel(const float *__restrict__ rgb, uint8_t *__restrict__ out,
                                                                   uint64_t pitch, int Wn, int H, int bottom_up, float exposure,
                                                                   uint32_t tiles_z, uint64_t tiles, SearchTree tab) {
    __shared__ float tree[256];
    __shared__ uint32_t image[kTileX * kPitch];
    const int t = (int)threadIdx.x;
    if (t < 256) tree[t] = tab.e[t];
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        __syncthreads();                                /* the tree is there; the tile before this one has been read */
        const int64_t z0 = (int64_t)(tile % tiles_z) * kTileZ, x0 = (int64_t)(tile / tiles_z) * kTileX;
        const int nz = (int)std::min<int64_t>(kTileZ, H - z0), nx = (int)std::min<int64_t>(kTileX, Wn - x0);

        /* in: lane = z, 16 columns a pass; every load of the thread is issued before the first is used */
        const int zl = t & (kTileZ - 1), xw = t / kTileZ;
        float v[kPerThread][3];
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int xl = k * (kThreads / kTileZ) + xw;
            v[k][0] = v[k][1] = v[k][2] = 0.0f;
            if (zl < nz && xl < nx) {
                const float *src = rgb + ((x0 + xl) * (int64_t)H + (z0 + zl)) * 3;
                v[k][0] = src[0], v[k][1] = src[1], v[k][2] = src[2];
            }
        }
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int xl = k * (kThreads / kTileZ) + xw;
            const uint32_t r = code_of(tree, v[k][0] * exposure), g = code_of(tree, v[k][1] * exposure),
                           b = code_of(tree, v[k][2] * exposure);
            image[xl * kPitch + zl] = r | (g << 8) | (b << 16) | 0xFF000000u;
        }
        __syncthreads();

        /* out: lane = x (C = 4) or a dword of the row (C = 3), 4 rows a pass */
        const int half = t / kTileX, j = t & (kTileX - 1);
#pragma unroll 4
        for (int k = 0; k < kTileZ * kTileX / kThreads; ++k) {
            const int zr = k * (kThreads / kTileX) + half;
            if (zr >= nz) continue;
            const int64_t z = z0 + zr, row = bottom_up ? z : (int64_t)H - 1 - z;
            uint8_t *dst = out + (uint64_t)row * pitch + (uint64_t)x0 * kC;
            if (kC == 4) {
                if (j < nx) *reinterpret_cast<uint32_t *>(dst + 4 * j) = image[j * kPitch + zr];
            } else {
                /* the row's 3 nx bytes start at any address: aligned dword j of them holds the row's bytes o0 .. o0 + 3 */
                const int n = 3 * nx, o0 = 4 * j - (int)((uintptr_t)dst & 3u);
                if (o0 >= 0 && o0 + 4 <= n) {
                    const int p0 = o0 / 3, s = o0 - 3 * p0, p1 = std::min(p0 + 1, kTileX - 1);
                    const uint64_t six = (uint64_t)(image[p0 * kPitch + zr] & 0xFFFFFFu) |
                                         ((uint64_t)(image[p1 * kPitch + zr] & 0xFFFFFFu) << 24);
                    *reinterpret_cast<uint32_t *>(dst + o0) = (uint32_t)(six >> (8 * s));
                } else {                                /* the row's two ends: the bytes it owns of a dword it shares */
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int o = o0 + b;
                        if (o >= 0 && o < n) dst[o] = (uint8_t)(image[(o / 3) * kPitch + zr] >> (8 * (o % 3)));
                    }
                }
            }
        }
    }
}

namespace {

bool builtin_table(int transfer, float *T /* [255] */) {
    if (transfer == RT_TRANSFER_SRGB) {
        std::memcpy(T, kSrgb, sizeof(kSrgb));
        return true;
    }
    if (transfer == RT_TRANSFER_LINEAR) {
        for (int k = 1; k <= 255; ++k) T[k - 1] = (float)((double)(2 * k - 1) / 510.0);
        return true;
    }
    return false;
}

/* the header's checks up to the buffers, in its order; on success *tab holds the transfer's thresholds */
int check_shape(const rt_image_params *p, int Wn, int H, uint64_t pitch, SearchTree *tab) {
    if (!p) return fail(RT_ERR_INVALID, "params is NULL");
    if (p->channels != 3 && p->channels != 4) return fail(RT_ERR_INVALID, "channels must be 3 or 4");
    if (p->bottom_up != 0 && p->bottom_up != 1) return fail(RT_ERR_INVALID, "bottom_up must be 0 or 1");
    if (p->transfer != RT_TRANSFER_SRGB && p->transfer != RT_TRANSFER_LINEAR && p->transfer != RT_TRANSFER_CUSTOM)
        return fail(RT_ERR_INVALID, "transfer is not one of RT_TRANSFER_*");
    if (!(p->exposure > 0.0f) || std::isinf(p->exposure)) return fail(RT_ERR_INVALID, "exposure must be finite and > 0");
    float T[255];
    if (!builtin_table(p->transfer, T)) {
        if (!p->thresholds) return fail(RT_ERR_INVALID, "thresholds is NULL");
        std::memcpy(T, p->thresholds, sizeof(T));
        for (int k = 0; k < 255; ++k)
            if (std::isnan(T[k])) return fail(RT_ERR_INVALID, "thresholds hold a NaN");
        for (int k = 1; k < 255; ++k)
            if (T[k] < T[k - 1]) return fail(RT_ERR_INVALID, "thresholds descend");
    }
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H * 3.0 > kMaxStripFloats) return fail(RT_ERR_INVALID, "strip too large");
    if (pitch < (uint64_t)Wn * (uint64_t)p->channels) return fail(RT_ERR_INVALID, "pitch_bytes is less than a row");
    if ((double)pitch * (double)H > kMaxOutBytes) return fail(RT_ERR_INVALID, "pitch_bytes * H too large");
    if (p->channels == 4 && (pitch & 3u) != 0) return fail(RT_ERR_INVALID, "pitch_bytes must be a multiple of 4 with 4 channels");
    tab->e[0] = 0.0f;
    for (int level = 1; level <= 8; ++level)
        for (int j = 0; j < (1 << (level - 1)); ++j) tab->e[(1 << (level - 1)) + j] = T[(((2 * j + 1) << (8 - level))) - 1];
    return RT_OK;
}

/* the one launch, enqueued on stream; every argument already checked, the device current */
int enqueue(const rt_image_params *p, const SearchTree &tab, int Wn, int H, const void *d_rgb, void *d_out, uint64_t pitch,
            hipStream_t stream) {
    const uint32_t tiles_z = (uint32_t)(((int64_t)H + kTileZ - 1) / kTileZ);
    const uint64_t tiles = (uint64_t)tiles_z * (uint64_t)(((int64_t)Wn + kTileX - 1) / kTileX);
    const dim3 grid((uint32_t)std::min<uint64_t>(tiles, kMaxBlocks));
    if (p->channels == 4)
        hipLaunchKernelGGL(rt_encode_image_kernel<4>, grid, dim3(kThreads), 0, stream, static_cast<const float *>(d_rgb),
                           static_cast<uint8_t *>(d_out), pitch, Wn, H, p->bottom_up, p->exposure, tiles_z, tiles, tab);
    else
        hipLaunchKernelGGL(rt_encode_image_kernel<3>, grid, dim3(kThreads), 0, stream, static_cast<const float *>(d_rgb),
                           static_cast<uint8_t *>(d_out), pitch, Wn, H, p->bottom_up, p->exposure, tiles_z, tiles, tab);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_image_version(void) { return RT_CAPI_IMAGE_VERSION; }

int rt_image_transfer_table(int transfer, float *out_T) {
    if (transfer == RT_TRANSFER_CUSTOM) return fail(RT_ERR_INVALID, "RT_TRANSFER_CUSTOM has no built-in table");
    if (transfer != RT_TRANSFER_SRGB && transfer != RT_TRANSFER_LINEAR)
        return fail(RT_ERR_INVALID, "transfer is not one of RT_TRANSFER_*");
    if (!out_T) return fail(RT_ERR_INVALID, "out_T is NULL");
    builtin_table(transfer, out_T);
    return RT_OK;
}

int rt_encode_image(int device, const rt_image_params *p, int Wn, int H, const float *rgb, uint8_t *out, uint64_t pitch_bytes,
                    double *kernel_ms) {
    SearchTree tab;
    int rc = check_shape(p, Wn, H, pitch_bytes, &tab);
    if (rc) return rc;
    if (!rgb || !out) return fail(RT_ERR_INVALID, "rgb / out is NULL");
    if ((rc = rt_internal_check_device(device))) return rc;
    /* on the device the rows are dense; the caller's pitch is applied by the copy back, row by row, so that the bytes between
     * its rows are never written */
    const size_t row_bytes = (size_t)Wn * (size_t)p->channels;
    const HostIn in[1] = {{rgb, (size_t)Wn * (size_t)H * 12}};
    const HostOut outs[1] = {{out, row_bytes * (size_t)H, row_bytes, (size_t)pitch_bytes}};
    return staged_call(device, in, 1, outs, 1, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        return enqueue(p, tab, Wn, H, d_in[0], d_out[0], row_bytes, nullptr);
    });
}

int rt_encode_image_device(int device, const rt_image_params *p, int Wn, int H, const void *d_rgb, void *d_out,
                           uint64_t pitch_bytes, void *hip_stream) {
    SearchTree tab;
    int rc = check_shape(p, Wn, H, pitch_bytes, &tab);
    if (rc) return rc;
    if (!d_rgb || !d_out) return fail(RT_ERR_INVALID, "d_rgb / d_out is NULL");
    if (((uintptr_t)d_rgb & 3u) != 0) return fail(RT_ERR_INVALID, "d_rgb must be 4-byte aligned");
    if (p->channels == 4 && ((uintptr_t)d_out & 3u) != 0) return fail(RT_ERR_INVALID, "d_out must be 4-byte aligned with 4 channels");
    const uint64_t in_bytes = (uint64_t)Wn * (uint64_t)H * 12;
    const uint64_t out_bytes = (uint64_t)(H - 1) * pitch_bytes + (uint64_t)Wn * (uint64_t)p->channels;
    if (overlap(d_rgb, in_bytes, d_out, out_bytes)) return fail(RT_ERR_INVALID, "d_out overlaps d_rgb");
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue(p, tab, Wn, H, d_rgb, d_out, pitch_bytes, static_cast<hipStream_t>(hip_stream));
}

} // extern "C"
