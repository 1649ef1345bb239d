/*
 * raytracer_main.cpp -- the counterpart of the reference's main() /
 * raytrace_main() (src/RayTracer.cpp:1122-1321, 855-1114): open the log,
 * build the hard-coded Scene and Camera, render every pixel, print the timing
 * lines, write raytracer_screen.txt.  The pixel loop itself
 * (src/RayTracer.cpp:904-923) is one call through the C ABI (rt_render /
 * rt_render_multi) into the HIP kernels; there is no CPU renderer here.
 *
 * With no arguments it runs the shipped configuration: SCENE 1, 500 x 504,
 * MAX_RECURSION_LEVEL 50 (src/rt_project_parameters.h:27,65-66,73).  The
 * reference fixes those at compile time; here they are run-time options:
 *   --width W --height H --depth D
 *   --scene 1 | 2 | grid:N | grid:N:noshadow
 *   --gpus G            x-strips over G GPUs, cut by measured cost, sent to GPU 0 with RCCL
 *   --out FILE          (default raytracer_screen.txt)   --no-txt
 *   --ssaa K            K x K samples per pixel, averaged in the render kernel (rt_render_ssaa; K = 1, 2, 4; one GPU)
 *   --hits FILE         also the W x H rt_hit records of the camera rays (rt_render_gbuffer: raw little-endian, 48 bytes each,
 *                       pixels[x][z] order); one GPU, no supersampling.  The .txt is the one written without it
 *   --denoise IT[:SIGMA[:K]]  filter the frame by its hit records before it is written (rt_render_gbuffer, then rt_denoise:
 *                       IT iterations 1..5, colour sigma SIGMA >= 0 (default 1.0), K normal squarings 0..6 (default 3)); one
 *                       GPU, no supersampling (a supersampled frame has no records)
 *   --ppm FILE          also the frame as a binary PPM, whatever made it (plain, --ssaa, --denoise, --gpus): rt_encode_image with
 *                       the sRGB table, 3 channels, the top row first (include/rt_capi_image.h)
 *   --exposure E        the colours are multiplied by E (finite, > 0; default 1) before they are encoded; needs --ppm
 *   --ao N[:RADIUS] --ao-ppm FILE   also the frame's ambient-occlusion plane as a binary PPM (include/rt_capi_ao.h): the camera
 *                       rays' records (rt_render_gbuffer), N x N directions per pixel (1..8) followed for RADIUS (default 1.0),
 *                       seed 0, three equal channels, encoded by rt_encode_image with the LINEAR table, the top row first; one
 *                       GPU, no supersampling.  The two options come together; the frame itself is the one rendered without them
 *   --adaptive K[:COLOR[:COS]]  K x K samples only for the pixels an edge passes through (rt_render_adaptive: K = 1, 2, 4; a pixel
 *                       is refined when it differs from another corner of its footprint in object, by a normal cosine below COS
 *                       (default 0.9, -1..1) or by more than COLOR in a colour channel (default 1/32, >= 0)); one GPU, instead
 *                       of --ssaa, without --hits, --denoise or --ao.  Composes with --ppm as --ssaa does
 *   --adaptive-mask FILE  also the refined pixels as a binary PGM (255: refined), the top row first; needs --adaptive
 *   --lens N[:APERTURE[:FOCUS[:SEED]]]  depth of field (rt_render_lens): N x N samples per pixel (1..8), each from its own point of a
 *                       lens of radius APERTURE (>= 0, default 0) through the focal plane at FOCUS times the screen's distance
 *                       (> 0, default 1), lens points hashed with SEED (default 0); one GPU, instead of --ssaa and --adaptive,
 *                       without --hits, --denoise or --ao.  Composes with --ppm and --out as --ssaa does
 *   --indirect N[:DEPTH[:GAIN[:SEED]]]  one diffuse bounce added to the frame (rt_render_gbuffer, then rt_indirect_diffuse on its
 *                       records with the frame as the base): N x N gather rays per pixel (1..8) traced at depth DEPTH (>= 0,
 *                       default 1), the term scaled by GAIN (finite, default 1), directions hashed with SEED (default 0); gather
 *                       rays that meet a light first count black (emitters 0).  One GPU, instead of --ssaa, --adaptive and
 *                       --lens, without --ao or --denoise.  Composes with --ppm and --out as --lens does
 *   --indirect-bounces B  with --indirect: every gather ray is followed for up to B bounces (1..8, default 1), one new direction
 *                       at every diffuse hit (rt_indirect_paths, include/rt_paths.h, in rt_indirect_diffuse's place; 1 is that
 *                       call itself).  An option of its own: a fifth field of --indirect stays the usage error it has been
 *   --indirect-compact  with --indirect: the term is computed by rt_indirect_paths_compact (include/rt_paths_compact.h) whatever B
 *                       is: the same frame bit for bit, only the paths still alive are traced at every bounce after the first,
 *                       and the host waits for the device once per bounce
 *   --gather-scale S[:SIGMA_PLANE[:refine]]  with --indirect or --ao: gather for every S-th pixel in both directions only (2..8)
 *                       and carry the term to every pixel by rt_upsample_guided (include/rt_capi_upsample.h: 3 normal squarings,
 *                       plane sigma SIGMA_PLANE >= 0, default 0: none); `refine`: the holes it reports are gathered at full
 *                       resolution afterwards, as one more batch with key0 0x80000000
 *   --accumulate K[:ALPHA]  K frames (1..65535) of the frame's own camera, the sampled term of the run -- --soft (through
 *                       rt_scene_set_shadow_seed), --ao or --indirect -- drawn with seeds 0..K-1, accumulated by
 *                       rt_temporal_accumulate (include/rt_temporal.h: normal cosine 0.9, plane distance 0.05, max_history K,
 *                       both blend weights at least ALPHA, 0..1, default 0: the running mean); the last accumulated frame (and
 *                       occlusion plane) is what the writers get.  One GPU, with at least one of those terms, without --ssaa,
 *                       --adaptive or --lens
 *   --svgf IT[:SIGMA_L[:MIN_HISTORY]]  with --accumulate: the last accumulated frame (and occlusion plane) goes through the
 *                       variance-steered filter before it is written (rt_svgf_filter, include/rt_svgf.h): IT iterations (1..5),
 *                       luminance sigma SIGMA_L (>= 0, default 2), spatial variance estimate below MIN_HISTORY frames (1..65535,
 *                       default 4) over a radius of 3; 3 normal squarings, the albedo matched, no plane term, epsilon 1e-8.  One
 *                       GPU, no supersampling
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/rt_capi.h"
#include "../../../include/rt_capi_adaptive.h"
#include "../../../include/rt_capi_ao.h"
#include "../../../include/rt_capi_denoise.h"
#include "../../../include/rt_capi_gbuffer.h"
#include "../../../include/rt_capi_image.h"
#include "../../../include/rt_capi_indirect.h"
#include "../../../include/rt_paths.h"
#include "../../../include/rt_paths_compact.h"
#include "../../../include/rt_capi_lens.h"
#include "../../../include/rt_capi_soft.h"
#include "../../../include/rt_capi_ssaa.h"
#include "../../../include/rt_svgf.h"
#include "../../../include/rt_temporal.h"
#include "../../../include/rt_capi_upsample.h"
#include "celio_model.hpp"
#include "screen_ppm.hpp"
#include "screen_txt.hpp"

using namespace CelioRayTracer;

/* the reference's file-scope state (src/RayTracer.h:44-52) */
static Scene my_scene = Scene();
static Camera my_camera = Camera();
static std::vector<float> pixels;          /* pixels[x][z] as packed fp32 RGB */

static int usage(const char *argv0) {
    std::fprintf(stderr,
                 "usage: %s [--width W] [--height H] [--depth D] [--scene 1|2|grid:N[:noshadow]]\n"
                 "          [--gpus G] [--out FILE] [--no-txt] [--ssaa 1|2|4] [--hits FILE] [--glass I:TF:IOR ...]\n"
                 "          [--soft I:N[:R] ...] [--denoise IT[:SIGMA[:K]]] [--ppm FILE [--exposure E]]\n"
                 "          [--ao N[:RADIUS] --ao-ppm FILE] [--adaptive 1|2|4[:COLOR[:COS]] [--adaptive-mask FILE]]\n"
                 "          [--lens N[:APERTURE[:FOCUS[:SEED]]]] [--indirect N[:DEPTH[:GAIN[:SEED]]]]\n"
                 "          [--indirect-bounces B] [--indirect-compact]\n"
                 "          [--gather-scale S[:SIGMA_PLANE[:refine]]] [--accumulate K[:ALPHA]]\n"
                 "          [--svgf IT[:SIGMA_L[:MIN_HISTORY]]]\n", argv0);
    return 1;
}

int main(int argc, char **argv) {
    int W = 500, H = 504, depth = 50, gpus = 1, ssaa = 1;
    bool write_txt = true, has_exposure = false;
    std::string scene_name = "1", out_path = "raytracer_screen.txt", hits_path, ppm_path, exposure_arg, ao_arg, ao_ppm_path;
    std::vector<std::string> glass;              /* --glass I:TF:IOR: object I refractive (include/rt_capi_refract.h) */
    std::string adaptive_arg, mask_path;         /* --adaptive K[:COLOR[:COS]], --adaptive-mask FILE (include/rt_capi_adaptive.h) */
    std::string lens_arg;                        /* --lens N[:APERTURE[:FOCUS[:SEED]]] (include/rt_capi_lens.h) */
    std::string indirect_arg;                    /* --indirect N[:DEPTH[:GAIN[:SEED]]] (include/rt_capi_indirect.h) */
    std::string bounces_arg;                     /* --indirect-bounces B (include/rt_paths.h) */
    bool indirect_compact = false;               /* --indirect-compact (include/rt_paths_compact.h) */
    std::string gather_arg;                      /* --gather-scale S[:SIGMA_PLANE[:refine]] (include/rt_capi_upsample.h) */
    bool has_gather = false;
    std::string accumulate_arg;                  /* --accumulate K[:ALPHA] (include/rt_temporal.h) */
    bool has_accumulate = false;
    std::string svgf_arg;                        /* --svgf IT[:SIGMA_L[:MIN_HISTORY]] (include/rt_svgf.h) */
    bool has_svgf = false;
    std::string denoise;                         /* --denoise IT[:SIGMA[:K]] (include/rt_capi_denoise.h) */
    std::vector<std::string> soft;               /* --soft I:N[:R]: light I an area light, N x N samples, radius R (include/rt_capi_soft.h) */
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](int &dst) { if (i + 1 >= argc) return false; dst = std::atoi(argv[++i]); return true; };
        if (a == "--width") { if (!need(W)) return usage(argv[0]); }
        else if (a == "--height") { if (!need(H)) return usage(argv[0]); }
        else if (a == "--depth") { if (!need(depth)) return usage(argv[0]); }
        else if (a == "--gpus") { if (!need(gpus)) return usage(argv[0]); }
        else if (a == "--ssaa") { if (!need(ssaa)) return usage(argv[0]); }
        else if (a == "--scene" && i + 1 < argc) scene_name = argv[++i];
        else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
        else if (a == "--hits" && i + 1 < argc) hits_path = argv[++i];
        else if (a == "--glass" && i + 1 < argc) glass.push_back(argv[++i]);
        else if (a == "--soft" && i + 1 < argc) soft.push_back(argv[++i]);
        else if (a == "--denoise" && i + 1 < argc) denoise = argv[++i];
        else if (a == "--ppm" && i + 1 < argc) ppm_path = argv[++i];
        else if (a == "--exposure" && i + 1 < argc) exposure_arg = argv[++i], has_exposure = true;
        else if (a == "--ao" && i + 1 < argc) ao_arg = argv[++i];
        else if (a == "--ao-ppm" && i + 1 < argc) ao_ppm_path = argv[++i];
        else if (a == "--adaptive" && i + 1 < argc) adaptive_arg = argv[++i];
        else if (a == "--adaptive-mask" && i + 1 < argc) mask_path = argv[++i];
        else if (a == "--lens" && i + 1 < argc) lens_arg = argv[++i];
        else if (a == "--indirect" && i + 1 < argc) indirect_arg = argv[++i];
        else if (a == "--indirect-bounces" && i + 1 < argc) bounces_arg = argv[++i];
        else if (a == "--indirect-compact") indirect_compact = true;
        else if (a == "--gather-scale" && i + 1 < argc) gather_arg = argv[++i], has_gather = true;
        else if (a == "--accumulate" && i + 1 < argc) accumulate_arg = argv[++i], has_accumulate = true;
        else if (a == "--svgf" && i + 1 < argc) svgf_arg = argv[++i], has_svgf = true;
        else if (a == "--no-txt") write_txt = false;
        else return usage(argv[0]);
    }
    if (W <= 0 || H <= 0 || depth < 0 || gpus <= 0) return usage(argv[0]);
    if ((ssaa != 1 && ssaa != 2 && ssaa != 4) || (ssaa > 1 && gpus > 1)) return usage(argv[0]);   /* (no multi-GPU supersampling) */
    if (!hits_path.empty() && (gpus > 1 || ssaa > 1)) return usage(argv[0]);   /* (G-buffers: one GPU, no supersampling) */
    rt_denoise_params dn = {0, 3, 1.0f};
    if (!denoise.empty()) {
        char tail = 0;
        const int got = std::sscanf(denoise.c_str(), "%d:%f:%d%c", &dn.iterations, &dn.sigma_color, &dn.normal_squarings, &tail);
        if (got < 1 || got > 3 || (got == 1 && denoise.find(':') != std::string::npos)) return usage(argv[0]);
        if (dn.iterations < 1 || dn.iterations > 5 || dn.normal_squarings < 0 || dn.normal_squarings > 6 ||
            !(dn.sigma_color >= 0.0f) || std::isinf(dn.sigma_color))
            return usage(argv[0]);
        if (gpus > 1 || ssaa > 1) return usage(argv[0]);       /* (one GPU; a supersampled frame has no records) */
    }
    rt_image_params im = {3, 0, RT_TRANSFER_SRGB, 1.0f, nullptr};
    if (has_exposure) {
        char *end = nullptr;
        im.exposure = std::strtof(exposure_arg.c_str(), &end);
        if (ppm_path.empty() || end == exposure_arg.c_str() || *end || !(im.exposure > 0.0f) || std::isinf(im.exposure))
            return usage(argv[0]);             /* (what rt_encode_image would refuse) */
    }
    rt_ao_params ao = {0, 1.0f, 0u, 0u, 3};
    if (ao_arg.empty() != ao_ppm_path.empty()) return usage(argv[0]);
    if (!ao_arg.empty()) {
        /* N, or N:RADIUS, and nothing else */
        char *end = nullptr;
        const long n = std::strtol(ao_arg.c_str(), &end, 10);
        if (end == ao_arg.c_str() || (*end != '\0' && *end != ':') || n < 1 || n > RT_AO_MAX_SAMPLES) return usage(argv[0]);
        ao.samples = (int)n;
        if (*end == ':') {
            const char *r = end + 1;
            ao.radius = std::strtof(r, &end);
            if (end == r || *end != '\0') return usage(argv[0]);
        }
        if (ao.samples < 1 || ao.samples > RT_AO_MAX_SAMPLES || !(ao.radius > 0.0f) || std::isinf(ao.radius)) return usage(argv[0]);
        if (gpus > 1 || ssaa > 1) return usage(argv[0]);       /* (one GPU; a supersampled frame has no records) */
    }
    rt_adaptive_params ad = {0, 0, 0, 1.0f / 32.0f, 0.9f};
    if (adaptive_arg.empty() && !mask_path.empty()) return usage(argv[0]);
    if (!adaptive_arg.empty()) {
        /* K, K:COLOR or K:COLOR:COS, and nothing else: what rt_render_adaptive would refuse is refused here */
        char *end = nullptr;
        const long k = std::strtol(adaptive_arg.c_str(), &end, 10);
        if (end == adaptive_arg.c_str() || (*end != '\0' && *end != ':') || (k != 1 && k != 2 && k != 4)) return usage(argv[0]);
        ad.samples = (int)k;
        float *fields[2] = {&ad.color_threshold, &ad.normal_cos};
        for (int f = 0; f < 2 && *end == ':'; ++f) {
            const char *v = end + 1;
            *fields[f] = std::strtof(v, &end);
            if (end == v || (*end != '\0' && (*end != ':' || f == 1))) return usage(argv[0]);
        }
        if (*end != '\0') return usage(argv[0]);
        if (!(ad.color_threshold >= 0.0f) || std::isinf(ad.color_threshold) || !(ad.normal_cos >= -1.0f && ad.normal_cos <= 1.0f))
            return usage(argv[0]);
        /* (one GPU; instead of --ssaa; the records stay inside the call) */
        if (gpus > 1 || ssaa > 1 || !hits_path.empty() || !denoise.empty() || !ao_arg.empty()) return usage(argv[0]);
    }
    rt_lens_params lens = {0, 0, 0u, 0.0f, 1.0f};
    if (!lens_arg.empty()) {
        /* N, N:APERTURE, N:APERTURE:FOCUS or N:APERTURE:FOCUS:SEED, and nothing else: what rt_render_lens would refuse is
         * refused here */
        char *end = nullptr;
        const long n = std::strtol(lens_arg.c_str(), &end, 10);
        if (end == lens_arg.c_str() || (*end != '\0' && *end != ':') || n < 1 || n > 8) return usage(argv[0]);
        lens.samples = (int)n;
        float *fields[2] = {&lens.aperture, &lens.focus};
        for (int f = 0; f < 2 && *end == ':'; ++f) {
            const char *v = end + 1;
            *fields[f] = std::strtof(v, &end);
            if (end == v || (*end != '\0' && *end != ':')) return usage(argv[0]);
        }
        if (*end == ':') {
            const char *v = end + 1;
            if (*v < '0' || *v > '9') return usage(argv[0]);                 /* (no sign, no blank) */
            const unsigned long long seed = std::strtoull(v, &end, 10);
            if (end == v || *end != '\0' || seed > 0xffffffffull) return usage(argv[0]);
            lens.seed = (uint32_t)seed;
        }
        if (*end != '\0') return usage(argv[0]);
        if (!(lens.aperture >= 0.0f) || std::isinf(lens.aperture) || !(lens.focus > 0.0f) || std::isinf(lens.focus))
            return usage(argv[0]);
        /* (one GPU; instead of --ssaa and --adaptive; a lens frame has no records) */
        if (gpus > 1 || ssaa > 1 || !adaptive_arg.empty() || !hits_path.empty() || !denoise.empty() || !ao_arg.empty())
            return usage(argv[0]);
    }
    rt_indirect_params ind = {0, 1, 0, 0, 0u, 0u, 1.0f};
    if (!indirect_arg.empty()) {
        /* N, N:DEPTH, N:DEPTH:GAIN or N:DEPTH:GAIN:SEED, and nothing else: what rt_indirect_diffuse would refuse is refused
         * here */
        char *end = nullptr;
        const long n = std::strtol(indirect_arg.c_str(), &end, 10);
        if (end == indirect_arg.c_str() || (*end != '\0' && *end != ':') || n < 1 || n > RT_INDIRECT_MAX_SAMPLES) return usage(argv[0]);
        ind.samples = (int)n;
        if (*end == ':') {
            const char *v = end + 1;
            if (*v < '0' || *v > '9') return usage(argv[0]);                 /* (no sign, no blank) */
            const long d = std::strtol(v, &end, 10);
            if (end == v || (*end != '\0' && *end != ':') || d > 0x7fffffffL) return usage(argv[0]);
            ind.gather_depth = (int)d;
        }
        if (*end == ':') {
            const char *v = end + 1;
            ind.gain = std::strtof(v, &end);
            if (end == v || (*end != '\0' && *end != ':')) return usage(argv[0]);
        }
        if (*end == ':') {
            const char *v = end + 1;
            if (*v < '0' || *v > '9') return usage(argv[0]);
            const unsigned long long seed = std::strtoull(v, &end, 10);
            if (end == v || *end != '\0' || seed > 0xffffffffull) return usage(argv[0]);
            ind.seed = (uint32_t)seed;
        }
        if (*end != '\0' || !std::isfinite(ind.gain)) return usage(argv[0]);
        /* (one GPU; instead of --ssaa, --adaptive and --lens; its records are the plain frame's) */
        if (gpus > 1 || ssaa > 1 || !adaptive_arg.empty() || !lens_arg.empty() || !denoise.empty() || !ao_arg.empty())
            return usage(argv[0]);
    }
    int bounces = 1;
    if (!bounces_arg.empty()) {
        /* B and nothing else, with --indirect: what rt_indirect_paths would refuse is refused here */
        char *end = nullptr;
        const long b = std::strtol(bounces_arg.c_str(), &end, 10);
        if (indirect_arg.empty() || bounces_arg[0] < '0' || bounces_arg[0] > '9' || *end != '\0' || b < 1 || b > RT_PATHS_MAX_BOUNCES)
            return usage(argv[0]);
        bounces = (int)b;
    }
    if (indirect_compact && indirect_arg.empty()) return usage(argv[0]);
    /* the indirect term of n records onto base (or alone): rt_indirect_diffuse, or with --indirect-bounces above 1
     * rt_indirect_paths of the same parameters, or with --indirect-compact rt_indirect_paths_compact of them */
    const auto indirect_term = [&](rt_scene *scene, const rt_indirect_params &g, int n, const rt_hit *records, const float *base,
                                   float *values) {
        if (bounces == 1 && !indirect_compact) return rt_indirect_diffuse(scene, &g, n, records, base, values);
        const rt_paths_params q = {g.samples, g.gather_depth, g.chunk_records, g.emitters, g.seed, g.key0, g.gain, bounces};
        if (indirect_compact) return rt_indirect_paths_compact(scene, &q, n, records, base, values);
        return rt_indirect_paths(scene, &q, n, records, base, values);
    };
    rt_upsample_params up = {0, 3, 3, 0, 0, 0.0f, 0.0f};
    bool refine = false;
    if (has_gather) {
        /* S, S:SIGMA_PLANE or S:SIGMA_PLANE:refine, and nothing else; with --indirect or --ao */
        char *end = nullptr;
        const long sc = std::strtol(gather_arg.c_str(), &end, 10);
        if (end == gather_arg.c_str() || (*end != '\0' && *end != ':') || sc < 2 || sc > 8) return usage(argv[0]);
        up.scale = (int)sc;
        if (*end == ':') {
            const char *v = end + 1;
            up.sigma_plane = std::strtof(v, &end);
            if (end == v || (*end != '\0' && *end != ':') || !(up.sigma_plane >= 0.0f) || std::isinf(up.sigma_plane))
                return usage(argv[0]);
            if (*end == ':') {
                if (std::strcmp(end + 1, "refine") != 0) return usage(argv[0]);
                refine = true;
            }
        }
        if (ao_arg.empty() && indirect_arg.empty()) return usage(argv[0]);
    }
    rt_temporal_params tp = {3, 0, 0, 0.9f, 0.05f, 0.0f, 0.0f};       /* max_history: K, 0 without --accumulate */
    if (has_accumulate) {
        /* K or K:ALPHA, and nothing else; one GPU, with a sampled term, the frame's records its own pixels' */
        char *end = nullptr;
        const long k = std::strtol(accumulate_arg.c_str(), &end, 10);
        if (end == accumulate_arg.c_str() || (*end != '\0' && *end != ':') || k < 1 || k > 65535) return usage(argv[0]);
        tp.max_history = (int)k;
        if (*end == ':') {
            const char *v = end + 1;
            tp.alpha = std::strtof(v, &end);
            if (end == v || *end != '\0' || !(tp.alpha >= 0.0f && tp.alpha <= 1.0f)) return usage(argv[0]);
            tp.alpha_moments = tp.alpha;
        }
        if (soft.empty() && ao_arg.empty() && indirect_arg.empty()) return usage(argv[0]);
        if (gpus > 1 || ssaa > 1 || !adaptive_arg.empty() || !lens_arg.empty()) return usage(argv[0]);
    }
    rt_svgf_params sv = {3, 0, 3, 1, 4, 3, 2.0f, 0.0f, 1e-8f};       /* iterations: IT, 0 without --svgf */
    if (has_svgf) {
        /* IT, IT:SIGMA_L or IT:SIGMA_L:MIN_HISTORY, and nothing else, refused as --denoise refuses its string */
        char tail = 0;
        const int got = std::sscanf(svgf_arg.c_str(), "%d:%f:%d%c", &sv.iterations, &sv.sigma_l, &sv.min_history, &tail);
        if (got < 1 || got > 3 || (got == 1 && svgf_arg.find(':') != std::string::npos)) return usage(argv[0]);
        if (sv.iterations < 1 || sv.iterations > 5 || sv.min_history < 1 || sv.min_history > 65535 || !(sv.sigma_l >= 0.0f) ||
            std::isinf(sv.sigma_l))
            return usage(argv[0]);
        if (!has_accumulate || gpus > 1 || ssaa > 1) return usage(argv[0]);   /* (it filters a history; one GPU, records needed) */
    }
    const int frames = has_accumulate ? tp.max_history : 1;
    /* a term gathered for the cells of the frame's records and upsampled onto `base` (or alone) into out, 3 channels: gather(n,
     * rows, records, key0, values) is the full-resolution call */
    auto gather_scaled = [&](const std::vector<rt_hit> &records, auto gather, int modulate, float dead_value, const float *base,
                             float *out, const char *what) -> int {
        const int Wl = (W + up.scale - 1) / up.scale, Hl = (H + up.scale - 1) / up.scale;
        std::vector<rt_hit> cells((size_t)Wl * (size_t)Hl);
        std::vector<float> lo(cells.size() * 3);
        std::vector<uint8_t> holes((size_t)W * (size_t)H);
        rt_upsample_params p = up;
        p.modulate = modulate, p.dead_value = dead_value;
        double up_ms = 0.0;
        int r = rt_subsample_hits(0, up.scale, 1, W, H, records.data(), cells.data());
        if (r == RT_OK) r = gather(Wl * Hl, Hl, cells.data(), 0u, lo.data());
        std::vector<float> kept;                     /* the base, where out overwrites it and the holes' add needs it */
        if (r == RT_OK && refine && base && base == out) kept.assign(base, base + records.size() * 3), base = kept.data();
        if (r == RT_OK) r = rt_upsample_guided(0, &p, W, H, records.data(), lo.data(), base, out, holes.data(), &up_ms);
        size_t n_holes = 0;
        for (uint8_t f : holes) n_holes += f;
        if (r == RT_OK)
            std::printf("%s at 1/%d density  : %d x %d cells, upsample kernel %f ms (plane sigma %g), %zu hole(s)%s\n", what,
                        up.scale * up.scale, Wl, Hl, up_ms, (double)up.sigma_plane, n_holes, refine ? ", refined" : "");
        if (r == RT_OK && refine && n_holes > 0) {
            std::vector<rt_hit> own;
            std::vector<size_t> where;
            for (size_t k = 0; k < holes.size(); ++k)
                if (holes[k]) own.push_back(records[k]), where.push_back(k);
            std::vector<float> term(own.size() * 3);
            r = gather((int)own.size(), (int)own.size(), own.data(), 0x80000000u, term.data());
            for (size_t k = 0; r == RT_OK && k < where.size(); ++k)
                for (int c = 0; c < 3; ++c)
                    out[where[k] * 3 + c] = base ? base[where[k] * 3 + c] + term[k * 3 + c] : term[k * 3 + c];
        }
        return r;
    };
    std::vector<uint8_t> mask;
    verbose() = true;                          /* console output like the reference's */

    if (gpus == 1) std::cout << "Single-Core RayTracing!" << std::endl << std::endl;
    else std::printf("\nMulti-Core RayTracing!\n\n");
    std::printf("  %d NUMBER OF CORES\n", gpus);

    /* raytrace_main(), src/RayTracer.cpp:855-1114 */
    std::printf("Global Rank(%d) begins\n", 0);
    const auto t_process = std::chrono::steady_clock::now();

    if (scene_name == "1") {
        if (my_scene.initialize()) return 1;
    } else if (scene_name == "2") {
        if (my_scene.initializeTwoMirrors(&my_camera)) return 1;
    } else if (scene_name.rfind("grid:", 0) == 0) {
        const std::string rest = scene_name.substr(5);
        const int n = std::atoi(rest.c_str());
        const bool shadows = rest.find(":noshadow") == std::string::npos;
        if (build_grid_scene(my_scene, my_camera, n, shadows)) {
            std::fprintf(stderr, "bad grid size\n");
            return 1;
        }
    } else {
        return usage(argv[0]);
    }

    for (const std::string &g : glass) {
        int idx = -1;
        float tf = 0.0f, ior = 1.0f;
        if (std::sscanf(g.c_str(), "%d:%f:%f", &idx, &tf, &ior) != 3 || idx < 0 || idx >= my_scene.getObjectCount())
            return usage(argv[0]);
        my_scene.getObject(idx)->getMaterial()->setRefractiveFactor(tf);
        my_scene.getObject(idx)->getMaterial()->setRefractiveIndex(ior);
    }

    for (const std::string &g : soft) {
        int idx = -1, n = 0;
        float r = -1.0f;                         /* (no R: the light's own radius) */
        const int got = std::sscanf(g.c_str(), "%d:%d:%f", &idx, &n, &r);
        if (got < 2 || idx < 0 || idx >= my_scene.getObjectCount() || !my_scene.getObject(idx)->checkIsaLightSource() || n < 1)
            return usage(argv[0]);
        my_scene.getObject(idx)->setAreaLight(n, r);
    }

    FlatScene flat;
    rt_camera_desc cam;
    my_scene.flatten(flat);
    my_camera.describe(cam);
    if (!flat.images.empty() && gpus > 1) {         /* the multi-GPU path takes no images (include/rt_capi_texture.h) */
        std::fprintf(stderr, "bitmap textures render on one GPU\n");
        return 1;
    }
    if (!flat.refractions.empty() && gpus > 1) {    /* nor refraction (include/rt_capi_refract.h) */
        std::fprintf(stderr, "refraction renders on one GPU\n");
        return 1;
    }
    if (!soft.empty() && gpus > 1) {                /* nor area lights (include/rt_capi_soft.h) */
        std::fprintf(stderr, "soft shadows render on one GPU\n");
        return 1;
    }
    pixels.assign((size_t)W * (size_t)H * 3, 0.0f);
    std::vector<rt_hit> hits(hits_path.empty() && denoise.empty() && ao_arg.empty() && indirect_arg.empty() && !has_accumulate
                                 ? 0 : (size_t)W * (size_t)H);
    std::vector<float> ao_plane(ao_arg.empty() ? 0 : (size_t)W * (size_t)H * 3);

    std::printf("****** Start Ray Tracing. *******\n");
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    double kernel_ms = 0.0;
    double camera_rays = (double)ssaa * (double)ssaa * (double)W * (double)H;       /* for the Mrays/s line */
    if (gpus == 1) {
        rt_scene *scene = nullptr;
        rc = flat.create(0, &scene);                /* with the scene's bitmap textures, refractions and area lights, if any */
        /* --accumulate: the history of the frame and of the occlusion plane, two sets each that take turns */
        struct History {
            std::vector<float> value[2], moments[2], length[2], variance;
        } frame_history, ao_history;
        double accumulate_ms = 0.0;
        auto accumulate = [&](History &h, std::vector<float> &cur, int k) -> int {
            const size_t n = (size_t)W * (size_t)H;
            const int to = k & 1, from = to ^ 1;
            h.value[to].resize(n * 3), h.moments[to].resize(n * 2), h.length[to].resize(n), h.variance.resize(n);
            double ms = 0.0;
            /* the camera does not move and the scene does not change: the previous frame's records are this frame's */
            const int r = rt_temporal_accumulate(0, &tp, k ? &cam : nullptr, &cam, W, H, 0, W, cur.data(), hits.data(),
                                                 k ? hits.data() : nullptr, k ? h.value[from].data() : nullptr,
                                                 k ? h.moments[from].data() : nullptr, k ? h.length[from].data() : nullptr,
                                                 h.value[to].data(), h.moments[to].data(), h.length[to].data(), h.variance.data(),
                                                 nullptr, &ms);
            accumulate_ms += ms;
            if (r == RT_OK) cur = h.value[to];
            return r;
        };
        for (int frame = 0; rc == RT_OK && frame < frames; ++frame) {
            if (has_accumulate) {
                ao.seed = ind.seed = (uint32_t)frame;
                if (!soft.empty()) rc = rt_scene_set_shadow_seed(scene, (uint32_t)frame);
            }
            if (rc != RT_OK) break;
            if (ad.samples > 0) {
                if (!mask_path.empty()) mask.assign((size_t)W * (size_t)H, 0);
                rc = rt_render_adaptive(scene, &cam, W, H, 0, W, depth, &ad, pixels.data(), mask.empty() ? nullptr : mask.data());
                rt_adaptive_info info;
                if (rc == RT_OK && rt_get_adaptive_info(scene, &info) == RT_OK) {
                    camera_rays += (double)info.rays;
                    std::printf("Adaptive supersampling     : %lld of %lld pixels refined (%.1f %%), %lld rays in %d launch(es); first pass "
                                "%f ms, flags %f ms, trace %f ms, resolve %f ms\n", (long long)info.flagged, (long long)info.pixels,
                                100.0 * (double)info.flagged / (double)info.pixels, (long long)info.rays, info.chunks, info.first_pass_ms,
                                info.flag_ms, info.trace_ms, info.resolve_ms);
                }
            } else if (lens.samples > 0) {
                rc = rt_render_lens(scene, &cam, W, H, 0, W, depth, &lens, pixels.data());
                rt_lens_info info;
                if (rc == RT_OK && rt_get_lens_info(scene, &info) == RT_OK) {
                    camera_rays = (double)info.rays;
                    std::printf("Lens camera                : %d x %d samples, aperture %g, focus %g, seed %u: %lld rays in %d chunk(s); "
                                "ray generation %f ms, trace %f ms, resolve %f ms\n", lens.samples, lens.samples, (double)lens.aperture,
                                (double)lens.focus, lens.seed, (long long)info.rays, info.chunks, info.raygen_ms, info.trace_ms,
                                info.resolve_ms);
                }
            } else {
                rc = ssaa > 1 ? rt_render_ssaa(scene, &cam, W, H, 0, W, depth, ssaa, pixels.data())
                   : !hits.empty() ? rt_render_gbuffer(scene, &cam, W, H, 0, W, depth, pixels.data(), hits.data())
                                   : rt_render(scene, &cam, W, H, 0, W, depth, pixels.data());
            }
            if (rc == RT_OK) {
                rt_timing tm;
                if (rt_get_timing(scene, &tm) == RT_OK) kernel_ms = tm.last_kernel_ms;
            }
            if (rc == RT_OK && !ao_arg.empty()) {           /* (before the filter: it reads the records, not the colours) */
                if ((double)W * (double)H > 533333333.0) {           /* (rt_ambient_occlusion's record limit; W * H must fit its int) */
                    std::fprintf(stderr, "--ao: the frame has more than 533333333 pixels\n");
                    rt_scene_destroy(scene);
                    return 1;
                }
                if (has_gather)
                    rc = gather_scaled(hits, [&](int n, int rows, const rt_hit *records, uint32_t key0, float *values) {
                             rt_ao_params a = ao;
                             a.key0 = key0;
                             return rt_ambient_occlusion(scene, &a, n, rows, records, values);
                         }, 0, 1.0f, nullptr, ao_plane.data(), "Ambient occlusion");
                else
                    rc = rt_ambient_occlusion(scene, &ao, W * H, H, hits.data(), ao_plane.data());
                rt_timing tm;
                if (rc == RT_OK && rt_get_timing(scene, &tm) == RT_OK)
                    std::printf("Ambient occlusion (ms)     : %f  (%d x %d directions, radius %g)\n", tm.last_kernel_ms, ao.samples,
                                ao.samples, (double)ao.radius);
            }
            if (rc == RT_OK && ind.samples > 0) {
                if ((double)W * (double)H > 533333333.0) {           /* (rt_indirect_diffuse's record limit; W * H must fit its int) */
                    std::fprintf(stderr, "--indirect: the frame has more than 533333333 pixels\n");
                    rt_scene_destroy(scene);
                    return 1;
                }
                if (has_gather)
                    rc = gather_scaled(hits, [&](int n, int, const rt_hit *records, uint32_t key0, float *values) {
                             rt_indirect_params g = ind;
                             g.key0 = key0;
                             return indirect_term(scene, g, n, records, nullptr, values);
                         }, 1, 0.0f, pixels.data(), pixels.data(), "Indirect diffuse ");
                else
                    rc = indirect_term(scene, ind, W * H, hits.data(), pixels.data(), pixels.data());
                rt_indirect_info info;
                rt_paths_info paths;
                rt_paths_compact_info compact;
                if (rc == RT_OK && indirect_compact && rt_get_paths_compact_info(scene, &compact) == RT_OK) {
                    std::printf("Indirect paths (compact)   : %d x %d paths of up to %d bounces at depth %d, gain %g, seed %u: %lld rays in %d "
                                "chunk(s), %d traces, %d queries, %d syncs; ray generation %f ms, trace %f ms, query %f ms, step %f ms, "
                                "resolve %f ms; alive", ind.samples, ind.samples, bounces, ind.gather_depth, (double)ind.gain, ind.seed,
                                (long long)compact.rays, compact.chunks, compact.traces, compact.queries, compact.syncs, compact.raygen_ms,
                                compact.trace_ms, compact.query_ms, compact.step_ms, compact.resolve_ms);
                    for (int b = 0; b < bounces; ++b) std::printf(" %lld", (long long)compact.alive[b]);
                    std::printf("\n");
                } else if (rc == RT_OK && bounces > 1 && rt_get_paths_info(scene, &paths) == RT_OK) {
                    std::printf("Indirect paths             : %d x %d paths of up to %d bounces at depth %d, gain %g, seed %u: %lld rays in %d "
                                "chunk(s); ray generation %f ms, trace %f ms, query %f ms, step %f ms, resolve %f ms; alive",
                                ind.samples, ind.samples, bounces, ind.gather_depth, (double)ind.gain, ind.seed, (long long)paths.rays,
                                paths.chunks, paths.raygen_ms, paths.trace_ms, paths.query_ms, paths.step_ms, paths.resolve_ms);
                    for (int b = 0; b < bounces; ++b) std::printf(" %lld", (long long)paths.alive[b]);
                    std::printf("\n");
                } else if (rc == RT_OK && rt_get_indirect_info(scene, &info) == RT_OK)
                    std::printf("Indirect diffuse           : %d x %d gather rays at depth %d, gain %g, seed %u: %lld rays in %d chunk(s); "
                                "ray generation %f ms, trace %f ms, query %f ms, resolve %f ms\n", ind.samples, ind.samples,
                                ind.gather_depth, (double)ind.gain, ind.seed, (long long)info.rays, info.chunks, info.raygen_ms,
                                info.trace_ms, info.query_ms, info.resolve_ms);
            }
            if (rc == RT_OK && has_accumulate) rc = accumulate(frame_history, pixels, frame);
            if (rc == RT_OK && has_accumulate && !ao_arg.empty()) rc = accumulate(ao_history, ao_plane, frame);
        }
        if (rc == RT_OK && has_accumulate) {
            double mean = 0.0;
            for (float v : frame_history.variance) mean += v;
            std::printf("Temporal accumulation      : %d frame(s), seeds 0..%d, alpha %g: kernels %f ms, mean luminance variance %g\n", frames,
                        frames - 1, (double)tp.alpha, accumulate_ms, mean / ((double)W * (double)H));
        }
        if (rc == RT_OK && sv.iterations > 0) {
            /* the last accumulated frame, and the occlusion plane's, through the variance-steered filter */
            const int to = (frames - 1) & 1;
            double svgf_ms = 0.0, ms = 0.0;
            rc = rt_svgf_filter(0, &sv, W, H, pixels.data(), hits.data(), frame_history.moments[to].data(),
                                frame_history.length[to].data(), pixels.data(), nullptr, nullptr, &svgf_ms);
            if (rc == RT_OK && !ao_arg.empty()) {
                rc = rt_svgf_filter(0, &sv, W, H, ao_plane.data(), hits.data(), ao_history.moments[to].data(),
                                    ao_history.length[to].data(), ao_plane.data(), nullptr, nullptr, &ms);
                svgf_ms += ms;
            }
            if (rc == RT_OK)
                std::printf("Variance-steered filter    : %f ms  (%d iteration(s), sigma_l %g, spatial estimate below %d frame(s))\n",
                            svgf_ms, sv.iterations, (double)sv.sigma_l, sv.min_history);
        }
        if (rc == RT_OK && !denoise.empty()) {
            double denoise_ms = 0.0;
            rc = rt_denoise(0, &dn, W, H, pixels.data(), hits.data(), pixels.data(), &denoise_ms);
            if (rc == RT_OK)
                std::printf("Denoise kernels (ms)       : %f  (%d iteration(s), sigma %g, %d normal squaring(s))\n", denoise_ms,
                            dn.iterations, (double)dn.sigma_color, dn.normal_squarings);
        }
        rt_scene_destroy(scene);
    } else {
        /* rt_render_multi() with the handle kept long enough to say how the image was cut: strips by measured cost, each
         * sent to GPU 0 in column chunks while the next chunk is rendered (rt_multi_render, chunks = 0) */
        rt_multi *multi = nullptr;
        rc = rt_multi_create(&flat.desc, gpus, &multi);
        if (rc == RT_OK) rc = rt_multi_render(multi, &cam, W, H, depth, 0, pixels.data());
        rt_multi_info info;
        if (rc == RT_OK && rt_multi_get_info(multi, &info) == RT_OK) {
            std::printf("Partition: %d x-strips of", info.ngpu);
            for (int g = 0; g < info.ngpu; ++g) {
                std::printf("%s%d", g ? "/" : " ", info.bounds[g + 1] - info.bounds[g]);
                if (info.kernel_ms[g] > kernel_ms) kernel_ms = info.kernel_ms[g];
            }
            if (info.transport == RT_MULTI_TRANSPORT_DIRECT)
                std::printf(" columns (%s), stored by the kernels straight into GPU 0's image; frame %f ms\n",
                            info.balanced ? "cut by measured cost" : "equal", info.frame_ms);
            else
                std::printf(" columns (%s), %d column chunk(s) per strip; frame %f ms\n",
                            info.balanced ? "cut by measured cost" : "equal", info.chunks, info.frame_ms);
        }
        rt_multi_destroy(multi);
    }
    if (rc != RT_OK) {
        std::fprintf(stderr, "render failed (%d): %s\n", rc, rt_last_error());
        return 1;
    }
    const auto t1 = std::chrono::steady_clock::now();
    /* The reference's Run_Time is CPU time since process start because its
     * start_time local shadows the global (src/RayTracer.cpp:893,1090); keep
     * "since process start" and also print the render-only figures. */
    const double run_time_s = std::chrono::duration<double>(t1 - t_process).count();
    const double render_s = std::chrono::duration<double>(t1 - t0).count();
    const double run_time_us = run_time_s * 1.0E6;
    std::printf("Finished.\n");
    std::printf("Total_Time (s) (Time.h)    : %f\n", run_time_s);
    std::printf("Render call (s)            : %f\n", render_s);
    if (kernel_ms > 0.0)
        std::printf("Render kernel (ms)         : %f  (%.1f Mrays/s)%s\n", kernel_ms,
                    camera_rays / (kernel_ms * 1e3), gpus > 1 ? "  [the GPU whose kernels took longest]" : "");
    std::printf("AverageRoundTime (us/pixel): %f\n", run_time_us / ((double)W * (double)H));

    if (!hits_path.empty()) {
        FILE *f = std::fopen(hits_path.c_str(), "wb");
        bool ok = f != nullptr;
        if (f) {
            ok = std::fwrite(hits.data(), sizeof(rt_hit), hits.size(), f) == hits.size();
            ok = std::fclose(f) == 0 && ok;
        }
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", hits_path.c_str());
            return 1;
        }
    }
    if (!ppm_path.empty()) {
        std::vector<uint8_t> image((size_t)W * (size_t)H * 3);
        double encode_ms = 0.0;
        if (rt_encode_image(0, &im, W, H, pixels.data(), image.data(), (uint64_t)W * 3u, &encode_ms) != RT_OK) {
            std::fprintf(stderr, "encode failed: %s\n", rt_last_error());
            return 1;
        }
        std::printf("Encode kernel (ms)         : %f  (sRGB, exposure %g)\n", encode_ms, (double)im.exposure);
        if (celio_write_screen_ppm(ppm_path.c_str(), W, H, image.data(), (uint64_t)W * 3u)) {
            std::fprintf(stderr, "cannot write %s\n", ppm_path.c_str());
            return 1;
        }
    }
    if (!mask_path.empty()) {
        /* the flags as a binary PGM, the top row (z = H - 1) first, like the PPM writers' scanlines */
        FILE *f = std::fopen(mask_path.c_str(), "wb");
        bool ok = f != nullptr;
        if (f) {
            std::vector<uint8_t> row((size_t)W);
            ok = std::fprintf(f, "P5\n%d %d\n255\n", W, H) > 0;
            for (int z = H - 1; ok && z >= 0; --z) {
                for (int x = 0; x < W; ++x) row[(size_t)x] = mask[(size_t)x * (size_t)H + (size_t)z] ? 255 : 0;
                ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
            }
            ok = std::fclose(f) == 0 && ok;
        }
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", mask_path.c_str());
            return 1;
        }
    }
    if (!ao_ppm_path.empty()) {
        const rt_image_params linear = {3, 0, RT_TRANSFER_LINEAR, 1.0f, nullptr};
        std::vector<uint8_t> image((size_t)W * (size_t)H * 3);
        if (rt_encode_image(0, &linear, W, H, ao_plane.data(), image.data(), (uint64_t)W * 3u, nullptr) != RT_OK) {
            std::fprintf(stderr, "encode failed: %s\n", rt_last_error());
            return 1;
        }
        if (celio_write_screen_ppm(ao_ppm_path.c_str(), W, H, image.data(), (uint64_t)W * 3u)) {
            std::fprintf(stderr, "cannot write %s\n", ao_ppm_path.c_str());
            return 1;
        }
    }
    if (write_txt) {
        std::printf("PrintScreen to Log.\n");
        std::printf("Greetings: %d, %d \n", W, H);
        if (celio_write_screen_txt(out_path.c_str(), W, H, pixels.data(), run_time_s,
                                   run_time_us / ((double)W * (double)H), gpus))
            return 1;
        std::printf("Closing log file.\n\n");
    }
    std::printf("Program Done.\n");
    return 0;
}
