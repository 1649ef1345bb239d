/*
 * ref_harness.cpp -- drives a build of the reference itself, for the tests.  TEST INFRASTRUCTURE ONLY.
 *
 * One translation unit: the reference's seven source files are included by path from the build copy that `make -C oracle ref`
 * puts under oracle/_ref/src (this file holds none of their text), compiled as they stand but for
 *   - the two stand-in headers beside this file (fixed_class.h, fixed_func.h), which the reference includes and does not ship;
 *   - MAX_RECURSION_LEVEL, a run-time int here (the reference uses it once, as an expression, in calculatePixel);
 *   - SCREEN_*_RESOLUTION, shrunk to 2: they size the static pixels[][] the harness does not use;
 *   - main, renamed (never called);
 *   - printf, routed to a counter of the reference's own "FAILURE" diagnostics, so that a scene that provokes one per ray
 *     does not write megabytes;
 *   - global operator new, which returns zeroed memory: CollisionObject::hitALightSource_Var is only ever set to true, so
 *     with zeroed memory every object the reference reads is defined.
 *
 *   ref_harness SCENE W H DEPTH OUT [MODE RAYS]
 *
 * SCENE: a text file of building verbs, one per line, every float as the 8 hex digits of its bit pattern:
 *   builtin | twomirrors | S o r | I o n h | C o vcorner hcorner | A o n h vdist hdist | color i c | diffuse i f |
 *   specular i f | reflective i f | checker i light dark w h | light i | intensity i f | indices RANK SIZE | cam2
 * Without MODE: the W x H frame, packed fp32 [x][z][3], through Camera::createEyeRay and calculatePixel as raytrace_main
 * calls them.  With MODE and RAYS (packed fp32 {E, T} per ray; W and H are ignored):
 *   trace     calculatePixel(Ray(E, T, E), 0)                                   -> 3 floats per ray
 *   hits      getCollision(Ray(E, T, E)) as an rt_hit (include/rt_capi_query.h) -> 48 bytes per ray
 *   occluded  inShadeCollisionDetection(Ray(E, T - E), |T - E|)                 -> 1 byte per ray
 * stdout: "failures N", the number of "FAILURE" diagnostics the reference printed.
 */
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <exception>
#include <iostream>
#include <new>
#include <string>
#include <vector>

void *operator new(size_t n) {
    void *p = calloc(n ? n : 1, 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void *operator new[](size_t n) { return operator new(n); }
void operator delete(void *p) noexcept { free(p); }
void operator delete[](void *p) noexcept { free(p); }
void operator delete(void *p, size_t) noexcept { free(p); }
void operator delete[](void *p, size_t) noexcept { free(p); }

static long ref_failures = 0;
static int ref_max_depth = 50;

static int ref_printf(const char *fmt, ...) {
    if (strstr(fmt, "FAILURE")) ref_failures++;
    return 0;
}

#include "rt_project_parameters.h"
#undef MAX_RECURSION_LEVEL
#define MAX_RECURSION_LEVEL ref_max_depth
#undef SCREEN_HORIZONTAL_RESOLUTION
#define SCREEN_HORIZONTAL_RESOLUTION 2
#undef SCREEN_VERTICAL_RESOLUTION
#define SCREEN_VERTICAL_RESOLUTION 2

#define printf ref_printf
#define main reference_main
#include "Camera.cpp"
#include "SceneObject.cpp"
#include "SceneSphere.cpp"
#include "SceneInfinitePlane.cpp"
#include "SceneFinitePlane.cpp"
#include "Scene.cpp"
#include "RayTracer.cpp"
#undef main
#undef printf

using CelioRayTracer::vector3d;

static void die(const char *what, const char *detail) {
    fprintf(stderr, "ref_harness: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
    exit(2);
}

static float hexf(const std::string &t) {
    char *end = NULL;
    unsigned long u = strtoul(t.c_str(), &end, 16);
    if (t.size() != 8 || *end) die("not an 8-hex-digit float", t.c_str());
    uint32_t b = (uint32_t)u;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

struct Line {
    std::vector<std::string> tok;
    size_t at;
    const std::string &next() {
        if (at >= tok.size()) die("too few fields after", tok[0].c_str());
        return tok[at++];
    }
    float f() { return hexf(next()); }
    int i() { return atoi(next().c_str()); }
    vector3d v() { float x = f(), y = f(), z = f(); return vector3d(x, y, z); }
};

static CelioRayTracer::SceneObject *object(int i) {
    if (i < 0 || i >= my_scene.getObjectCount()) die("object index out of range", NULL);
    return my_scene.getObject(i);
}

static void build_scene(const char *path) {
    FILE *fp = fopen(path, "r");
    if (!fp) die("cannot open scene", path);
    char buf[1024];
    while (fgets(buf, sizeof buf, fp)) {
        Line l;
        l.at = 1;
        for (char *t = strtok(buf, " \t\r\n"); t; t = strtok(NULL, " \t\r\n")) l.tok.push_back(t);
        if (l.tok.empty() || l.tok[0][0] == '#') continue;
        const std::string &verb = l.tok[0];
        if (verb == "builtin") {
            if (my_scene.initialize()) die("Scene::initialize failed", NULL);
        } else if (verb == "twomirrors") {
            if (my_scene.initializeTwoMirrors(&my_camera)) die("Scene::initializeTwoMirrors failed", NULL);
        } else if (verb == "S") {
            vector3d o = l.v();
            my_scene.addObject(new CelioRayTracer::SceneSphere(o, l.f()));
        } else if (verb == "I") {
            vector3d o = l.v(), n = l.v(), h = l.v();
            my_scene.addObject(new CelioRayTracer::SceneInfinitePlane(o, n, h));
        } else if (verb == "C") {
            vector3d o = l.v(), vc = l.v(), hc = l.v();
            my_scene.addObject(new CelioRayTracer::SceneFinitePlane(o, vc, hc));
        } else if (verb == "A") {
            vector3d o = l.v(), n = l.v(), h = l.v();
            float vd = l.f(), hd = l.f();
            my_scene.addObject(new CelioRayTracer::SceneFinitePlane(o, n, h, vd, hd));
        } else if (verb == "color") {
            int i = l.i();
            object(i)->getMaterial()->setColor(l.v());
        } else if (verb == "diffuse") {
            int i = l.i();
            object(i)->getMaterial()->setDiffuseFactor(l.f());
        } else if (verb == "specular") {
            int i = l.i();
            object(i)->getMaterial()->setSpecularFactor(l.f());
        } else if (verb == "reflective") {
            int i = l.i();
            object(i)->getMaterial()->setReflectiveFactor(l.f());
        } else if (verb == "checker") {
            int i = l.i();
            vector3d light = l.v(), dark = l.v();
            float w = l.f(), h = l.f();
            CelioRayTracer::ObjTexture *t = new CelioRayTracer::Texture_CheckerBoard(light, dark);
            t->setWidth(w);
            t->setHeight(h);
            object(i)->getMaterial()->setTexture(t);
        } else if (verb == "light") {
            object(l.i())->setAsLightSource();
        } else if (verb == "intensity") {
            int i = l.i();
            object(i)->setIntensity(l.f());
        } else if (verb == "indices") {
            int rank = l.i(), size = l.i();
            my_scene.SetObjectIndices(rank, size);
        } else if (verb == "cam2") {
            my_camera.setSceneTwoMirrors();
        } else {
            die("unknown verb", verb.c_str());
        }
    }
    fclose(fp);
}

static std::vector<float> read_rays(const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) die("cannot open rays", path);
    fseek(fp, 0, SEEK_END);
    long bytes = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (bytes < 0 || bytes % 24) die("rays file is not a whole number of {E, T} records", path);
    std::vector<float> rays(bytes / 4);
    if (bytes && fread(rays.data(), 1, bytes, fp) != (size_t)bytes) die("short read", path);
    fclose(fp);
    return rays;
}

/* the rt_hit of include/rt_capi_query.h */
struct Hit {
    int32_t object;
    float distance, point[3], normal[3], color[3];
    int32_t flags;
};

static void put(float *dst, vector3d v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }

/* CollisionObject keeps no usable index: the winner is the lowest object whose own collision() reports the winner's distance
 * (getCollision replaces its candidate only on a strictly smaller one) */
static int winner_index(Ray *ray, float distance) {
    for (int x = 0; x < my_scene.getObjectCount(); x++) {
        CollisionObject *c = my_scene.getObject(x)->collision(ray);
        if (!c) continue;
        bool same = c->getDistance() == distance;
        delete c;
        if (same) return x;
    }
    return -1;
}

int main(int argc, char **argv) {
    if (argc != 6 && argc != 8) {
        fprintf(stderr, "usage: %s SCENE W H DEPTH OUT [trace|hits|occluded RAYS]\n", argv[0]);
        return 2;
    }
    int W = atoi(argv[2]), H = atoi(argv[3]);
    ref_max_depth = atoi(argv[4]);
    build_scene(argv[1]);
    FILE *out = fopen(argv[5], "wb");
    if (!out) die("cannot open output", argv[5]);

    if (argc == 6) {
        if (W < 1 || H < 1) die("bad frame size", NULL);
        std::vector<float> frame((size_t)W * H * 3);
        for (int x = 0; x < W; x++) {
            for (int z = 0; z < H; z++) {
                Ray *ray = my_camera.createEyeRay(((float)x) / W, ((float)z) / H);
                put(&frame[((size_t)x * H + z) * 3], calculatePixel(ray, 0));
                free(ray);
            }
        }
        fwrite(frame.data(), 4, frame.size(), out);
    } else {
        std::string mode = argv[6];
        std::vector<float> rays = read_rays(argv[7]);
        size_t n = rays.size() / 6;
        for (size_t k = 0; k < n; k++) {
            const float *r = &rays[k * 6];
            vector3d E(r[0], r[1], r[2]), T(r[3], r[4], r[5]);
            if (mode == "trace") {
                Ray ray(E, T, E);
                float rgb[3];
                put(rgb, calculatePixel(&ray, 0));
                fwrite(rgb, 4, 3, out);
            } else if (mode == "hits") {
                Ray ray(E, T, E);
                Hit h;
                memset(&h, 0, sizeof h);
                h.object = -1;
                CollisionObject *c = getCollision(&ray);
                if (c) {
                    h.distance = c->getDistance();
                    put(h.point, c->getIntersectionPoint());
                    put(h.normal, c->getNormalRay().getDirection());
                    put(h.color, c->getColor());
                    h.flags = (c->insideHit() ? 1 : 0) | (c->hitALightSource() ? 2 : 0);
                    h.object = winner_index(&ray, h.distance);
                    delete c;
                }
                fwrite(&h, sizeof h, 1, out);
            } else if (mode == "occluded") {
                vector3d dir;
                dir = T - E;
                float dist_to_light = dir.length();
                Ray lightRay(E, dir);
                unsigned char verdict = inShadeCollisionDetection(&lightRay, dist_to_light) ? 1 : 0;
                fwrite(&verdict, 1, 1, out);
            } else {
                die("unknown mode", mode.c_str());
            }
        }
    }
    if (fclose(out)) die("write failed", argv[5]);
    fprintf(stdout, "failures %ld\n", ref_failures);
    return 0;
}
