/*
 * The host side of rt_lens.hip (include/rt_capi_lens.h) -- everything that needs no device: the argument checks in the header's
 * order and the chunk arithmetic -- as a program of its own, for AddressSanitizer (scripts/asan_lens_host.sh).  It includes the
 * unit itself, so that the functions of its unnamed namespace can be called; on a machine without a GPU every entry point stops
 * at the device question.  Exit status 0: every expectation held (the sanitizer aborts on its own findings).
 */
#include "../tilecoderaytracer_amd/csrc/rt_lens.hip"

#include <cstdio>
#include <limits>

static int failures = 0;

#define EXPECT(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, rt_last_error()); \
            ++failures;                                                                       \
        }                                                                                     \
    } while (0)

static bool said(const char *word) { return std::string(rt_last_error()).find(word) != std::string::npos; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const rt_lens_params good = {2, 0, 0u, 0.25f, 8.0f};
    /* the params' checks, each field's bad values with every later field bad as well */
    EXPECT(check_params(nullptr, 4, 3) == RT_ERR_INVALID && said("params"));
    EXPECT(check_params(&good, 4, 3) == RT_OK);
    const rt_lens_params bad[] = {{9, -2, 0u, -1.0f, 0.0f}, {0, 0, 0u, 0.0f, 1.0f}, {2, -2, 0u, -1.0f, 0.0f}, {2, 0, 0u, -1.0f, 0.0f},
                                  {2, 0, 0u, nan, 0.0f},   {2, 0, 0u, inf, 1.0f},  {2, 0, 0u, 0.0f, 0.0f},   {2, 0, 0u, 0.0f, nan},
                                  {2, 0, 0u, 0.0f, inf},   {2, 0, 0u, 0.0f, -2.0f}};
    const char *word[] = {"samples", "samples", "chunk_columns", "aperture", "aperture", "aperture", "focus", "focus", "focus", "focus"};
    for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
        EXPECT(check_params(&bad[i], 1 << 30, 1 << 30) == RT_ERR_INVALID);            /* (the virtual size is bad as well) */
        EXPECT(said(word[i]));
    }
    const rt_lens_params ends[] = {{1, 0, 0u, 0.0f, 1.0e-30f}, {8, 2147483647, 4294967295u, 3.0e38f, 3.0e38f}};
    for (const rt_lens_params &p : ends) EXPECT(check_params(&p, 4, 3) == RT_OK);
    EXPECT(check_params(&good, 1 << 30, 3) == RT_ERR_INVALID && said("2^31"));
    EXPECT(check_params(&good, 3, 1 << 30) == RT_ERR_INVALID && said("2^31"));
    EXPECT(check_params(&good, (1 << 30) - 1, (1 << 30) - 1) == RT_OK);

    /* the ray generation's checks, then the device question */
    rt_camera_desc cam = {};
    std::vector<float> rays((size_t)4 * 3 * 4 * 6, 9.0f);
    EXPECT(rt_lens_rays(&cam, 0, 3, 0, 0, &bad[0], 0, nullptr) == RT_ERR_INVALID && said("x0 <= x1"));
    EXPECT(rt_lens_rays(nullptr, 4, 3, 0, 4, &bad[0], 0, nullptr) == RT_ERR_INVALID && said("NULL") && !said("camera"));
    EXPECT(rt_lens_rays(nullptr, 4, 3, 0, 4, &bad[0], 0, rays.data()) == RT_ERR_INVALID && said("camera"));
    EXPECT(rt_lens_rays(&cam, 4, 3, 0, 4, nullptr, 0, rays.data()) == RT_ERR_INVALID && said("params"));
    EXPECT(rt_lens_rays(&cam, 4, 3, 0, 4, &bad[0], 0, rays.data()) == RT_ERR_INVALID && said("samples"));
    const rt_lens_params eight = {8, 0, 0u, 0.25f, 8.0f};
    EXPECT(rt_lens_rays(&cam, 1 << 15, 1 << 15, 0, 1 << 15, &eight, 0, rays.data()) == RT_ERR_INVALID && said("rays"));
    EXPECT(rt_lens_rays_device(&cam, 4, 3, 0, 4, &good, 0, (void *)0x10002, nullptr) == RT_ERR_INVALID && said("4-byte"));
    const int rc = rt_lens_rays(&cam, 4, 3, 0, 4, &good, 0, rays.data());
    EXPECT(rc == RT_ERR_NO_DEVICE || rc == RT_OK);
    if (rc == RT_ERR_NO_DEVICE) EXPECT(rays.front() == 9.0f && rays.back() == 9.0f);   /* nothing was written */
    const int rc_empty = rt_lens_rays(&cam, 4, 3, 2, 2, &good, 0, nullptr);
    EXPECT(rc_empty == RT_ERR_NO_DEVICE || rc_empty == RT_OK);

    /* the frame call without a scene: rt_render's refusal, whatever else is wrong */
    std::vector<float> rgb(4 * 3 * 3, 0.5f);
    EXPECT(rt_render_lens(nullptr, &cam, 4, 3, 0, 4, 1, &bad[0], rgb.data()) == RT_ERR_INVALID);
    EXPECT(std::string(rt_last_error()) == "scene is NULL");
    EXPECT(rt_render_lens_device(nullptr, nullptr, 0, 0, 5, 1, -1, nullptr, nullptr, nullptr) == RT_ERR_INVALID);
    rt_lens_info info;
    EXPECT(rt_get_lens_info(nullptr, &info) == RT_ERR_INVALID);

    /* the chunk arithmetic: the default keeps rays and sample colours within 256 MiB and has at least one column, no chunk has
     * more rays than a ray batch takes or more columns than the strip, and the chunks of any strip cover it exactly */
    rt_lens_params p = good;                                             /* S = 4 */
    EXPECT(chunk_columns(p, 4096, 4096) == 455 && 455LL * 4096 * 4 * 36 <= (long long)kChunkBytes &&
           456LL * 4096 * 4 * 36 > (long long)kChunkBytes);
    p.samples = 4;
    EXPECT(chunk_columns(p, 4096, 4096) == 113);
    p.samples = 8;
    EXPECT(chunk_columns(p, 1 << 20, 100) == 1);                          /* a column beyond 256 MiB: one column still */
    EXPECT(chunk_columns(p, (int)(kMaxBatchRays / 64), 100) == 1);        /* the tallest column check (8) lets through */
    p.chunk_columns = 2147483647;
    EXPECT(chunk_columns(p, 4096, 4096) == 4096);                         /* 2^30 rays: within a batch */
    EXPECT(chunk_columns(p, 4096, 20000) == (int)(kMaxBatchRays / (4096LL * 64)));
    for (int n : {1, 2, 3, 8}) {
        for (int chunk : {0, 1, 7, 61, 1000}) {
            for (int columns : {1, 6, 7, 8, 61, 4096}) {
                p.samples = n, p.chunk_columns = chunk;
                const int H = 37, c = chunk_columns(p, H, columns);
                EXPECT(c >= 1 && c <= columns && (long long)c * H * n * n <= kMaxBatchRays);
                if (chunk > 0) EXPECT(c == std::min(chunk, columns));
                int covered = 0, chunks = 0;
                for (int xc = 0; xc < columns; xc += c) covered += std::min(c, columns - xc), ++chunks;
                EXPECT(covered == columns && chunks == (columns + c - 1) / c);
            }
        }
    }
    EXPECT(blocks_of(1) == 1 && blocks_of(256) == 1 && blocks_of(257) == 2);
    EXPECT(lds_floats() == 3328 && lds_stride(4) == 13 && lds_stride(9) == 27 && lds_stride(64) == 193);
    for (int n = 1; n <= kMaxSamples; ++n) EXPECT((kResolveSamples / (n * n)) * lds_stride(n * n) <= lds_floats());

    /* a fresh state: nothing to collect, nothing timed, freed without a device */
    RtLensState *a = new RtLensState();
    EXPECT(collect(a) == RT_OK && lens_ms(a, 0) < 0.0);
    lens_free(a);
    lens_free(nullptr);

    std::printf(failures ? "asan_lens_host: %d expectation(s) failed\n" : "asan_lens_host: ok\n", failures);
    return failures ? 1 : 0;
}
