/*
 * rt_tables.h -- the device scene format: what rt_scene_create() packs from an
 * rt_scene_desc and what every workgroup stages into LDS.
 *
 * The image is an array of 16-byte "quads" (float4).  Sections, in order:
 *
 *   geometry   one record per object; Scene index order, except that the
 *              spheres of a clustered run are stored leaf by leaf
 *                sphere          1 quad : {cx, cy, cz, r^2}
 *                infinite plane  5 quads: q0 {n.xyz, distance_to_origin}
 *                finite plane    5 quads  q1 {anchor.xyz, h_distance}
 *                                         q2 {horizontal.xyz, v_distance}
 *                                         q3 {vertical.xyz, 0}
 *                                         q4 {reverseNormal.xyz, 0}
 *                (anchor = SceneObject::origin for the infinite plane,
 *                 plane_origin for the finite plane: the point texture/bounds
 *                 coordinates are measured from)
 *   aa         2 quads per axis-aligned finite plane (its fast test record):
 *                {dto, sn, sh, sv}, {po_a, po_b, h_dist, v_dist}
 *                in coordinates permuted to (normal, horizontal, vertical) axis
 *   cidx       one u32 per clustered sphere: its Scene index (member order)
 *   near items, shadow items   2 quads per ITEM, see below
 *   lights     2 quads per light, Scene index order:
 *                {origin.xyz, intensity}, {colour.rgb, bits(object index)}
 *   materials  2 quads per DISTINCT (ObjMaterial, intensity, light flag) row:
 *                {colour.rgb, diffuse}, {specular, reflective, intensity,
 *                 bits(is_light | (texture+1) << 1)}
 *   textures   2 quads per checkerboard: {light.rgb, width}, {dark.rgb, height}; in a scene with images
 *              (include/rt_capi_texture.h) instead 2 quads per texture, checkerboards first, each one packed as its 2 x 2
 *              CHECKER image: {width, height, bits(texels_w), bits(texels_h)}, {bits(wrap), 0, bits(the image's block in the
 *              texel buffer: low word), bits(high word)}; a block is texels_w x texels_h rgb fp32 texels, then the column
 *              bounds b_0 .. b_(texels_w - 1), then the row bounds (rt_kernel.hip, image_cell())
 *   refraction (scenes with refractive objects only: include/rt_capi_refract.h) one header quad right before the materials,
 *              {bits(offset of the rows), 0, 0, 0}, and behind the textures one quad per material row: {tf, ior, 0, 0}
 *   soft       (scenes with area lights only: include/rt_capi_soft.h) the same header quad, its y word bits(offset of the rows),
 *              and behind the refraction rows (if any) one quad per light: {r, step, bits(n), r'}
 *   objinfo    one u32 per object (4 per quad):
 *                bits 0-15 geometry offset (quads), 16-17 kind, 20-31 material row
 *
 * Clustered sphere runs.  A run of >= 4*leaf consecutive spheres is regrouped
 * (k-d median split of the centres) into spatial leaves of <= leaf spheres.  A leaf's
 * box is axis-aligned, inflated, and contains every member sphere.  Members are visited out of Scene order; the nearest hit
 * stays exact because ties are broken on the Scene index (the lexicographic
 * minimum of (distance, index) is what an in-order scan with a strict `<`
 * computes).
 *
 * Items.  Both scans of the reference -- getCollision over all objects
 * (src/RayTracer.cpp:50-89) and the shadow scan over the non-light objects of
 * the scan range (src/RayTracer.cpp:709-739) -- walk a table of ITEMS: one per
 * object that is not in a clustered run, in Scene index order, then one per
 * LEAF of each clustered run.  2 quads per item:
 *   {box CENTRE.xyz, bits(kind | count << 8 | geometry quad offset << 16)},
 *   {box HALF-EXTENT.xyz, bits(Scene index | quad offset of the full 5-quad plane record << 12)}
 * (the box is [centre - half, centre + half]; an axis the item is unbounded on: centre 0, half-extent infinity)
 * kind = RT_KIND_SPHERE / _INFINITE_PLANE / _FINITE_PLANE;
 *        RT_KIND_FINITE_AA + normal axis for an axis-aligned rectangle (geometry
 *        offset = its aa record);
 *        RT_KIND_SPHERE_LEAF for a leaf (count = its members, geometry offset =
 *        its first member sphere, second word = u32 index of its members'
 *        Scene indices).
 * The box (inflated on the host) contains the object; an infinite plane's box
 * is all of space.  The wavefront culls 64 item boxes at once, one per lane
 * (rt_kernel.hip: nearest_hit_items, in_shade).
 */
#ifndef RT_TABLES_H_
#define RT_TABLES_H_

#include <stdint.h>

#define RT_SPHERE_QUADS 1
#define RT_PLANE_QUADS  5
#define RT_LIGHT_QUADS  2
#define RT_MAT_QUADS    2
#define RT_TEX_QUADS    2
/* A light's rows: {position.xyz, intensity}, {colour.xyz, bits(Scene index | flags)}.  RT_LIGHT_COLOURS_WILD, the same in every
 * row of a scene: some light's colour has a component that is not finite -- then no product with a light's colour is known to
 * be +-0 (rt_kernel.hip, SPECULAR GATE).  RT_SCENE_VALUES_WILD, likewise in every row: some colour component (an object's, a
 * checkerboard's, the null colour's), factor (diffuse, specular, reflective) or intensity of the scene is a NaN, infinite or of
 * magnitude above 1 -- then a reflected ray's colour is not known to be finite (rt_kernel.hip, DEAD REFLECTIONS).  Both are 0
 * in a scene with neither: its rows are what they were before the flags existed. */
#define RT_LIGHT_COLOURS_WILD 0x80000000u
#define RT_SCENE_VALUES_WILD  0x40000000u

/* item kinds: RT_KIND_* of rt_capi.h (0 sphere, 1 infinite plane, 2 finite
 * plane), plus axis-aligned finite planes: kind = 4 + axis of the normal (0 x, 1 y, 2 z).
 * Their 2-quad test record lists the two in-plane axes in cyclic order after the
 * normal's: {dto, sign_n, sign_a, sign_b}, {origin_a, origin_b, extent_a, extent_b}.
 * The full 5-quad record of each plane is kept too (winner record, non-finite rays). */
#define RT_KIND_FINITE_AA 4
/* one leaf of a clustered sphere run as an item: count = its members, geometry
 * offset = its first member sphere, second word = u32 index of its members'
 * Scene indices */
#define RT_KIND_SPHERE_LEAF 10
#define RT_AA_QUADS 2
/* bit 4 of an item's first word: the item is a finite plane, whose box is padded for a plane's rounding only
 * and whose slack in the wavefront culls is RT_PLANE_SLACK of the distance instead of RT_SPHERE_SLACK */
#define RT_ITEM_TIGHT 16u

#define RT_MAX_GEOM_QUADS 65535   /* 16-bit geometry offset in objinfo */
#define RT_MAX_MATERIALS  4095    /* 12-bit material row in objinfo    */
#define RT_MAX_OBJECTS    4096    /* 12-bit Scene index in the item tables */
#define RT_MAX_LDS_BYTES  (160 * 1024)
#ifndef RT_LDS_TABLE_BYTES
#define RT_LDS_TABLE_BYTES (80 * 1024)   /* automatic: larger tables than this stay in global memory (rt_render_kernel_large) */
#endif
#ifndef RT_STACK_LDS_SHARE
#define RT_STACK_LDS_SHARE 7      /* tables + the LDS part of the bounce stack must fit this many times per CU */
#endif

#define RT_TILE_STATS 6          /* counting build: words per wavefront tile {cycles, sphere tests, box tests, scans, start, end (100 MHz clock)} */

/* tile queues: one per XCD, heads RT_QUEUE_STRIDE words apart (own cache lines);
 * a macro tile is RT_MACRO_ROWS vertically adjacent wavefront tiles */
#define RT_TILE_QUEUES 8
#define RT_QUEUE_STRIDE 32
/* a launch's block of counters: the eight queue heads and the HEAVY tiles' head, each on its own cache line.  Every launch
 * zeroes the block its scene's NEXT launch will use (RtParams::next_counters) */
#define RT_COUNTER_WORDS ((RT_TILE_QUEUES + 1) * RT_QUEUE_STRIDE)
#ifndef RT_MACRO_ROWS
#define RT_MACRO_ROWS 4
#endif
#define RT_GETREG_XCC_ID ((3 << 11) | (0 << 6) | 20)   /* s_getreg_b32 HW_REG_XCC_ID, bits [3:0] */

#define RT_HELP_LEAVES 8
#define RT_HELP_SPIN_LIMIT (1 << 22)
#define RT_HEAVY_PERMILLE10 25        /* automatic half-width of the HEAVY band: 0.25 % of the image height (2 tile rows of 4 pixels at 4096) */
/* the workgroup's HELP desk: words of LDS (rt_kernel.hip) */
enum { RT_DESK_STATE = 0, RT_DESK_CURSOR, RT_DESK_INSIDE, RT_DESK_FINISHED, RT_DESK_MASK_LO, RT_DESK_MASK_HI,
       RT_DESK_BASE, RT_DESK_VERDICT_LO, RT_DESK_VERDICT_HI, RT_DESK_BROKEN, RT_DESK_DEDICATED, RT_DESK_PHASE, RT_DESK_WORDS = 12 };

#define RT_NEAR_CULL_MIN_ITEMS 8     /* below this many items the nearest scan skips the bundle cull */
#define RT_SHADOW_CULL_MIN_ITEMS 8   /* below this many shadow items the wavefront skips the bundle-box cull */

#ifndef RT_ORDER_MIN_CANDIDATES
#define RT_ORDER_MIN_CANDIDATES 4    /* from this many candidates on the nearest scan takes them nearest first */
#endif

#define RT_STACK_ENTRY_BYTES 16   /* {local.rgb, bits(object index | texsel << 16)} per bounce level per lane */

/* IMAGE TEXTURES (include/rt_capi_texture.h; the *_image kernels only).  Only planes get a textured material row there (a
 * sphere's texture is dropped), and the texel selector of a hit is the index of its texel within its image (< 2^20, the
 * scene's texel limit).  A bounce-stack entry is {local.rgb, bits(object index | texsel << 12)}: 12 bits of object index
 * (RT_MAX_OBJECTS), 20 of selector. */
#define RT_IMAGE_SEL_SHIFT 12

/* REFRACTION (include/rt_capi_refract.h; the *_refract kernels only, whose scenes are always packed as image scenes).  One more
 * section, one quad per material row: {tf, ior, 0, 0}; its quad offset is bits of the x word of the quad right before the
 * materials.  A level's bounce-stack entry is three quads: {local or partial.rgb, bits(object index | texsel << 12)},
 * {transmitted origin.xyz, bits(state)}, {transmitted direction.xyz, 0}; state 0: the reflected child is walked, 1: the
 * transmitted child, 2: the reflected child with the transmitted one pending. */
#define RT_REFR_QUADS 1
#define RT_REFRACT_ENTRY_QUADS 3

/* SOFT SHADOWS (include/rt_capi_soft.h; the *_soft and *_refract_soft kernels only, whose scenes are always packed as image
 * scenes).  One more section, one quad per light in light order: {r, step = 2 / n, bits(n), r' = r (1 + 2^-10) rounded up}; a
 * light that is not an area light has {0, 2, bits(1), 0} and keeps the hard shadow.  Its quad offset is bits of the y word of
 * the header quad right before the materials (the one whose x word holds the refraction rows' offset; 0 there when the scene
 * has no refraction).  The launch's sampling seed is not in the image: the *_soft kernels take it as one more kernel argument
 * behind the ones every render kernel shares (RENDER KERNELS, below). */
#define RT_SOFT_QUADS 1

#define RT_PRIMARY_ITEMS 64          /* scenes with more FAST items than this have no PRIMARY table */

/* relative growth of a leaf's box that must contain every member sphere the reference's float arithmetic can report from a
 * given origin (derived at box_needed(), rt_kernel.hip); the host's SHADOW VOXELS use the same figure */
#ifndef RT_SPHERE_SLACK
#define RT_SPHERE_SLACK 1.5e-3f
#endif
/* SHADOW VOXELS (below): at most this many voxels, lights and shadow items */
#ifndef RT_SVOX_MAX_CELLS
#define RT_SVOX_MAX_CELLS 4096
#endif
/* cells beyond the core, per axis and side: cell j holds the points whose distance d beyond the core, in core cells, has
 * 16^j <= 1 + 15 d < 16^(j+1) -- four cells reach 4 369 core cells out; further away every item may matter anyway */
#define RT_SVOX_TAIL 4
#define RT_SVOX_MAX_LIGHTS 2        /* one quad per voxel: a 64-bit mask per light */
#define RT_SVOX_MAX_ITEMS 64
#define RT_SVOX_MIN_LEAVES 24        /* automatic: scenes with fewer leaves get no table (option "svox" n: from 4 leaves on) */

typedef struct RtParams {
    /* camera (src/Camera.cpp:71-84) */
    float so[3], ch[3], cv[3], eye[3];
    float sw, sh, shw, shh;
    float null_color[3];
    int32_t W, H, x0, x1, max_depth;
    /* tables */
    int32_t n_lights;
    int32_t n_shadow_items, shadow_items_off;            /* shadow item table (quads), see below */
    int32_t n_near_items, near_items_off;                /* nearest-hit item table                      */
    int32_t n_clusters;                                  /* leaves of clustered sphere runs       */
    int32_t near_first_leaf, shadow_first_leaf;          /* item tables: the leaf items are the ones from this index on (the tables' ends if none) */
    int32_t image_quads;                 /* quads staged into LDS */
    int32_t lights_off, mat_off, tex_off, objinfo_off;   /* quad offsets */
    /* tiling: a wavefront renders tile_x x tile_z pixels, tile_x * tile_z == 64 */
    int32_t tile_z_log2;
    int32_t tiles_z;                     /* wavefront tiles along z */
    int32_t tiles_x;                     /* wavefront tiles along x */
    int32_t n_tiles;                     /* total wavefront tiles   */
    int32_t stack_off;                   /* quad offset of the bounce stack's LDS levels: behind the tables, or 0 when the tables stay in global memory */
    int32_t stack_stride;                /* threads that keep a bounce stack per workgroup (all of them) */
    int32_t stack_lds_levels;            /* bounce levels below this keep their stack entries in LDS (behind the tables), the others in HBM */
    int32_t first_macro_row;             /* the tile queues start at this macro row and wrap around ... */
    int32_t rows_downwards;              /* ... upwards (0) or downwards (1)                           */
    /* HELP (rt_kernel.hip): the workgroup's desk, RT_DESK_WORDS words of LDS at quad desk_off; help_rays_quads != 0:
     * the launch carries 128 quads of global memory per workgroup for the published rays (0: no helping) */
    int32_t desk_off, help_rays_quads;
    int32_t help_leaves;                 /* a shadow scan with this many candidate leaves asks for help (RT_HELP_LEAVES; option "help") */
    int32_t help_spin_limit;             /* the owner's bounded wait for helpers to leave its desk (RT_HELP_SPIN_LIMIT; < 0: every wait counts as timed out -- tests) */
    /* HEAVY tiles (rt_kernel.hip): the tiles within heavy_half tile rows of the horizon line -- tile row
     * (heavy_row0_q16 + tile column * heavy_slope_q16) >> 16 -- are rendered first, one per WORKGROUP: wavefront 0
     * renders, the others serve its shadow scans at the desk from the first scan on.  heavy_half < 0: none. */
    int32_t heavy_half, heavy_row0_q16, heavy_slope_q16;
    /* OLD TILES FIRST (rt_kernel.hip): a wavefront's priority on its SIMD rises with the age of its tile (0: off) */
    int32_t tile_prio;
    int32_t cull;                        /* 0: plain in-order scans (no bundle cull, no nearest-first exit); option "cull" */
    /* FAST tables (scenes without clustered sphere runs, option "fast"): see below */
    int32_t n_fast_items, n_fast_shadow; /* items in all; the first n_fast_shadow are the shadow scan's */
    int32_t fast_box_off, fast_rec_off;  /* quad offsets: 2 box quads and 2 record quads per item */
    int32_t fast_ctl_off;                /* u32 offset (4 per quad): one control word per item */
    /* PRIMARY table (FAST tables, at most RT_PRIMARY_ITEMS items; rt_capi.hip: primary_table()): per item of the FAST list, for
     * THIS launch's camera and image, the rectangle of pixels whose camera ray can reach the item's box and a lower bound of the
     * distance at which it does: the nearest-hit scan of the camera rays needs no bundle bounds, no reciprocals and no box
     * arithmetic -- a tile is a pixel rectangle.  n_primary = items (0: no table, the camera rays take the general cull);
     * primary_off = its place in LDS (quads, behind the image; one quad per item: {x_lo | x_hi << 16 (int16 pixels),
     * z_lo | z_hi << 16, bits of the entry distance, 0}). */
    int32_t n_primary, primary_off;
    /* SHADOW VOXELS (scenes with clustered sphere runs, at most RT_SVOX_MAX_ITEMS shadow items and RT_SVOX_MAX_LIGHTS lights;
     * rt_capi.hip: shadow_voxels(); option "svox").  A grid of svox_n[0] x [1] x [2] voxels over the part of space the leaves
     * occupy (the core), continued on every axis and side by RT_SVOX_TAIL cells that grow 16-fold each (N = n + 2 RT_SVOX_TAIL
     * cells per axis); per voxel and light one 64-bit mask: bit i set = shadow item i can block the segment from SOME
     * point of the voxel to that light (plain items: always set; a leaf: its box, grown by the slack the float sphere test needs
     * from anywhere in the voxel, meets the hull of voxel and light).  A shadow scan ORs the masks of its lanes' voxels (a lane
     * outside the grid: all ones) and ANDs the result into the candidates its bundle cull left: the bundle is one box around
     * all 64 shading points, the voxels follow each ray.  svox_off = quad offset of the table in the image's GLOBAL copy, behind
     * the part that is staged into LDS (0: no table); one quad per voxel (light 0's mask, light 1's), voxel = (z * Ny + y) * Nx + x, the
     * per-axis cell numbers as svox_axis_cell() (rt_kernel.hip) finds them from (P.k - svox_lo[k]) * svox_scale[k] */
    int32_t svox_off;
    int32_t svox_n[3];
    float svox_lo[3], svox_scale[3];
    uint32_t primary[RT_PRIMARY_ITEMS * 4];
    /* one word of host memory the kernel can write (rt_scene's sticky device error): set when a HELP wait timed out */
    uint64_t error_word;
    /* the block of counters (RT_COUNTER_WORDS u32) this scene's next launch will use: this launch zeroes its heads */
    uint64_t next_counters;
    /* diagnostic (option "timeline"): 0, or device memory for RT_TIMELINE_WORDS u64 per wavefront tile, row-major:
     * {start, end (100 MHz constant clock), workgroup * 16 + wavefront, 1 if rendered as a HEAVY tile} */
    uint64_t timeline;
    /* SUPERSAMPLING (include/rt_capi_ssaa.h; the *_ssaa kernels only): log2 k of k x k samples per output pixel.  Every other
     * field describes the VIRTUAL kW x kH launch; the store averages each pixel's samples into the W x H output.  (Last, so
     * that no other field moves; padded to 16 bytes, so that the kernel arguments behind the struct keep their kernarg
     * offsets modulo 16: the scalar loads of those merge as before, and the other kernels' code differs in those offsets only.) */
    int32_t ssaa_log2;
    /* RAY BATCH (include/rt_capi_rays.h; the *_rays kernels only): n_rays rays of {E.xyz, T.xyz} fp32 at device address `rays`,
     * ray i at cell (i / H, i % H) of a W x H launch (W = x1 = n_cols, x0 = 0); no camera, no PRIMARY table.  (Where ssaa_pad[3]
     * was: `rays` at offset 1344 is 8-aligned, so no other field moves and the struct keeps its 1352 bytes.)
     * G-BUFFER (include/rt_capi_gbuffer.h; the *_gbuffer kernels only): gbuffer_hits is the device address of the strip's
     * rt_hit records, 48 bytes per pixel in the colours' order, 16-byte aligned.  A camera launch never reads `rays`, so the
     * two share one place and nothing moves. */
    int32_t n_rays;
    union {
        uint64_t rays;
        uint64_t gbuffer_hits;
    };
} RtParams;
#define RT_TIMELINE_WORDS 4

/* RAY QUERIES (include/rt_capi_query.h): what a ray-batch launch computes -- colours (rt_trace_rays), the *_hits kernels'
 * 48-byte records or the *_occluded kernels' one-byte verdicts.  A template argument of the kernels and the host's choice of
 * sibling, not an RtParams field. */
enum { RT_QUERY_NONE = 0, RT_QUERY_HITS = 1, RT_QUERY_OCCLUDED = 2, RT_QUERY_AO = 3 };
#define RT_HIT_BYTES 48

/* FAST tables.  Scenes without clustered sphere runs (the reference's built-in Scene: 32 objects) are walked
 * through ONE item list that serves both scans: first the objects of the shadow scan (the non-light objects of
 * the scan range), then the others; within each part sorted by kind.  Neither scan depends on the order: the
 * shadow verdict is an OR (src/RayTracer.cpp:727-729), the nearest hit the minimum of (distance, Scene index)
 * (:71-80).  Per item i:
 *   box      2 quads {centre.xyz, bits(kind | RT_ITEM_TIGHT)}, {half-extent.xyz, control word}: what the wavefront culls test
 *   record   2 quads, all the exact test reads, so that a candidate costs ONE LDS round trip:
 *              sphere          {c.xyz, r^2}, {-}
 *              infinite plane  {n.xyz, distance_to_origin}, {-}
 *              AA rectangle    {dto, sn, sa, sb}, {origin_a, origin_b, extent_a, extent_b}   (as RT_KIND_FINITE_AA)
 *              finite plane    {n.xyz, distance_to_origin}, {bits(quad offset of its full record), -, -, -}
 *   control  one u32: kind | Scene index << 8, read with a SCALAR load from the image in global memory (the
 *            wavefront's dispatch on the kind and the index for ties never touch a vector register) */
#define RT_FAST_BOX_QUADS 2
#define RT_FAST_REC_QUADS 2

/* RENDER KERNELS.  Every render kernel but the two counting ones (rt_render_kernel_stats, _fast_stats) is
 * rt_render_kernel<mode><family>: one of the five TABLE MODES below times one of the FAMILIES after them, all of it the one
 * body of rt_kernel.hip (render_body<kStats = false, kGlobalTables, kClusters, kRoomy, kFast, kSsaa, kRays, kQuery, kGbuffer,
 * kImages, kRefract, kSoft>).  rt_kernel.hip defines them, rt_capi.hip declares them and picks one per launch
 * (choose_kernel()); both expand these lists, so a new family is one line here plus the host's family rule.
 *
 * RT_TABLE_MODES(X, family...): X(mode suffix, kGlobalTables, kClusters, kRoomy, kFast, workgroup bound, wavefronts per SIMD,
 * wavefronts per SIMD of the soft families, family...) -- the launch bounds' names are rt_kernel.hip's.
 *   ""              FAST tables (scenes without clustered sphere runs; the built-in scene, the bench headline): 72 VGPRs, seven
 *                   wavefronts per SIMD where LDS allows (the bounce stack keeps its LDS place up to seven workgroups per CU,
 *                   RT_STACK_LDS_SHARE).  The base family's kernel of this mode, rt_render_kernel, is the TWIN TILES kernel
 *                   (below): 96 VGPRs, five wavefronts per SIMD, its own bound RT_WAVES_PER_SIMD_TWIN
 *   _items          the same over the two item tables: option "fast" = 0, and option "cull" = 0 (the plain in-order scans)
 *   _large          scenes whose tables are large (or do not fit LDS at all): the tables stay in global memory.  These need
 *                   52-62 VGPRs and so run 8 wavefronts per SIMD although their bound asks for RT_WAVES_PER_SIMD only; the
 *                   sample loop would take their soft siblings to 72 registers and 7 wavefronts, so those ask for the 8 their
 *                   siblings reach (no *_soft kernel runs below its sibling's occupancy)
 *   _clusters       scenes with clustered sphere runs (PAIRS, NEAREST PAIRS, HELP, HEAVY tiles): 80 registers, six wavefronts per
 *                   SIMD (workgroups of up to eight wavefronts: scenes whose tables are large share one LDS copy among more of
 *                   them, launch_block() in rt_capi.hip)
 *   _clusters_wide  the same with the registers of five wavefronts per SIMD, for scenes whose tables leave room for no more
 *                   than five workgroups per CU anyway (the 1 024-sphere grid: 31.5 KB); the pair flush tests four members
 *                   abreast here */
#define RT_TABLE_MODES(X, ...)                                                                                                \
    X(,               false, false, false, true,  RT_BLOCK_BOUND,          RT_WAVES_PER_SIMD,          RT_WAVES_PER_SIMD,          __VA_ARGS__) \
    X(_items,         false, false, false, false, RT_BLOCK_BOUND,          RT_WAVES_PER_SIMD,          RT_WAVES_PER_SIMD,          __VA_ARGS__) \
    X(_large,         true,  false, false, false, RT_BLOCK_BOUND,          RT_WAVES_PER_SIMD,          8,                          __VA_ARGS__) \
    X(_clusters,      false, true,  false, false, RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS, __VA_ARGS__) \
    X(_clusters_wide, false, true,  true,  false, RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE,     RT_WAVES_PER_SIMD_WIDE,     __VA_ARGS__)

/* TWIN TILES.  rt_render_kernel -- the FAST tables' kernel of the camera's plain frame, the bench headline -- renders wavefront
 * tiles in vertical pairs: every lane carries two pixels, one of each of tile rows 2j and 2j + 1 of a macro tile, and what a
 * wavefront does as a whole (bundle bounds, culls, candidate order, scalar dispatch) runs once for both (rt_kernel.hip,
 * render_tile_twin(), on render_tile()'s per-ray routines).  A queue entry is a twin, its bounce stack has two rows per level, and its launch bound
 * is RT_WAVES_PER_SIMD_TWIN instead of the mode's.  Every other kernel renders one tile per wavefront, and so does this one
 * with -DRT_TWIN_TILES=0 (a build switch, not an option: both bodies in one kernel would cost both their registers).
 * RT_KERNEL_IS_TWIN: the rule, from a kernel's catalogue columns, for rt_kernel.hip and rt_capi.hip alike. */
#ifndef RT_TWIN_TILES
#define RT_TWIN_TILES 1
#endif
#define RT_KERNEL_IS_TWIN(global_tables, clusters, fast, ssaa, rays, query, gbuffer, images, refract, soft)                    \
    (RT_TWIN_TILES != 0 && (fast) && !(global_tables) && !(clusters) && !(ssaa) && !(rays) && (query) == RT_QUERY_NONE &&      \
     !(gbuffer) && !(images) && !(refract) && !(soft))

/* The families, one list per translation unit of kernels: rt_kernel.hip is compiled once per unit (-DRT_KERNEL_TU=<unit>,
 * rt_kernel_<unit>.o; the base unit is rt_kernel.o), each unit's kernels in this order.  The split is part of the speed
 * contract: next to more instances of the body in one module the item-table kernel's register allocation moved (one more
 * spilled scalar), and a unit of its own keeps each kernel's code what it is alone.
 * X(family suffix, kSsaa, kRays, kQuery, kGbuffer, kImages, kRefract, kSoft, takes the sampling seed)
 *   base     the camera's frame
 *   ssaa     include/rt_capi_ssaa.h: the virtual kW x kH image of k x k samples per pixel, averaged at the store
 *   rays     include/rt_capi_rays.h: a caller's rays instead of a camera's
 *   query    include/rt_capi_query.h: one question per ray of a batch -- getCollision's record, or a segment's shadow verdict
 *   gbuffer  include/rt_capi_gbuffer.h: a camera's frame and, beside each pixel, the rt_hit record of its camera ray
 *   texture  include/rt_capi_texture.h: the *_image sibling of the above but the occlusion query (which reads no colour)
 *   refract  include/rt_capi_refract.h: the *_refract sibling of the colour families, the image body walking a ray tree
 *   soft     include/rt_capi_soft.h: the *_soft and *_refract_soft siblings, the image body sampling area lights; the
 *            launch's sampling seed is one more kernel argument behind the shared ones (RT_SEED_PARAM_true), so RtParams
 *            and the other kernels' arguments do not change */
#define RT_UNIT_base(X)     X(,                      false, false, RT_QUERY_NONE,     false, false, false, false, false)
#define RT_UNIT_ssaa(X)     X(_ssaa,                 true,  false, RT_QUERY_NONE,     false, false, false, false, false)
#define RT_UNIT_rays(X)     X(_rays,                 false, true,  RT_QUERY_NONE,     false, false, false, false, false)
#define RT_UNIT_query(X)    X(_hits,                 false, true,  RT_QUERY_HITS,     false, false, false, false, false) \
                            X(_occluded,             false, true,  RT_QUERY_OCCLUDED, false, false, false, false, false)
#define RT_UNIT_gbuffer(X)  X(_gbuffer,              false, false, RT_QUERY_NONE,     true,  false, false, false, false)
#define RT_UNIT_texture(X)  X(_image,                false, false, RT_QUERY_NONE,     false, true,  false, false, false) \
                            X(_ssaa_image,           true,  false, RT_QUERY_NONE,     false, true,  false, false, false) \
                            X(_rays_image,           false, true,  RT_QUERY_NONE,     false, true,  false, false, false) \
                            X(_hits_image,           false, true,  RT_QUERY_HITS,     false, true,  false, false, false) \
                            X(_gbuffer_image,        false, false, RT_QUERY_NONE,     true,  true,  false, false, false)
#define RT_UNIT_refract(X)  X(_refract,              false, false, RT_QUERY_NONE,     false, true,  true,  false, false) \
                            X(_ssaa_refract,         true,  false, RT_QUERY_NONE,     false, true,  true,  false, false) \
                            X(_rays_refract,         false, true,  RT_QUERY_NONE,     false, true,  true,  false, false) \
                            X(_gbuffer_refract,      false, false, RT_QUERY_NONE,     true,  true,  true,  false, false)
#define RT_UNIT_soft(X)     X(_soft,                 false, false, RT_QUERY_NONE,     false, true,  false, true,  true)  \
                            X(_ssaa_soft,            true,  false, RT_QUERY_NONE,     false, true,  false, true,  true)  \
                            X(_rays_soft,            false, true,  RT_QUERY_NONE,     false, true,  false, true,  true)  \
                            X(_gbuffer_soft,         false, false, RT_QUERY_NONE,     true,  true,  false, true,  true)  \
                            X(_refract_soft,         false, false, RT_QUERY_NONE,     false, true,  true,  true,  true)  \
                            X(_ssaa_refract_soft,    true,  false, RT_QUERY_NONE,     false, true,  true,  true,  true)  \
                            X(_rays_refract_soft,    false, true,  RT_QUERY_NONE,     false, true,  true,  true,  true)  \
                            X(_gbuffer_refract_soft, false, false, RT_QUERY_NONE,     true,  true,  true,  true,  true)
#define RT_RENDER_FAMILIES(X)                                                                                                 \
    RT_UNIT_base(X) RT_UNIT_ssaa(X) RT_UNIT_rays(X) RT_UNIT_query(X) RT_UNIT_gbuffer(X) RT_UNIT_texture(X) RT_UNIT_refract(X) \
    RT_UNIT_soft(X)

/* The render kernels' arguments.  `help_area`: the clustered-scene kernels' HELP areas (128 quads of global memory per
 * workgroup for the rays a wavefront publishes at its workgroup's desk); unused by the others.  The counting kernels have
 * `stats_out` before it; a family that takes the sampling seed has it last (RT_SEED_PARAM_<takes the seed>). */
#define RT_KERNEL_ARGS                                                                                            \
    const RtParams p_in_kernarg, const float4 *__restrict__ image, float *__restrict__ out,                      \
    unsigned int *__restrict__ tile_counter, float4 *__restrict__ bounce_stack, unsigned int *__restrict__ help_area
#define RT_KERNEL_ARGS_STATS                                                                                      \
    const RtParams p_in_kernarg, const float4 *__restrict__ image, float *__restrict__ out,                      \
    unsigned int *__restrict__ tile_counter, float4 *__restrict__ bounce_stack,                                   \
    unsigned long long *__restrict__ stats_out, unsigned int *__restrict__ help_area
#define RT_SEED_PARAM_false
#define RT_SEED_PARAM_true , const uint32_t shadow_seed

/* AUXILIARY KERNELS: kernels that are the same body over the same tables in the five table modes, but no render kernels -- they
 * are not rt_render_kernel<mode><family>, not in RT_RENDER_FAMILIES, and their list is RT_AUX_UNIT_<unit> (the render families'
 * columns): rt_kernel_<unit>.o is built with -DRT_KERNEL_AUX_TU=<unit>.  There is one:
 *   ao   include/rt_capi_ao.h: AMBIENT OCCLUSION, rt_ao_kernel<mode> -- a query over a batch of rt_hit RECORDS instead of rays
 *        (RtParams::rays is the records' address, n_rays their number): n x n hemisphere segments of length R per record, each
 *        one the occlusion query's scan.  n, R, key0 and the output's channels are kernel arguments of these kernels only
 *        (RT_AO_PARAMS, handed to render_body() as an RtAoArgs); the seed travels as RT_SEED_PARAM_true does. */
typedef struct RtAoArgs { int32_t samples; float radius; uint32_t key0; int32_t channels; } RtAoArgs;
#define RT_AUX_UNIT_ao(X)   X(,                      false, true,  RT_QUERY_AO,       false, false, false, false, true)
#define RT_AO_PARAMS , const int32_t ao_samples, const float ao_radius, const uint32_t ao_key0, const int32_t ao_channels

#endif /* RT_TABLES_H_ */
