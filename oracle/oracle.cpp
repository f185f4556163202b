/*
 * oracle.cpp — CPU ORACLE.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library; the product (misaki-render_amd/) never links, imports or
 * calls it and has no CPU fallback.
 *
 * What it is: a scalar C++ restatement of misaki-render's sampling hot path
 *     SamplingIntegrator::render -> render_block -> render_sample
 *       -> PathTracer::sample -> Scene::ray_intersect / ray_test
 *       -> ImageBlock::put -> Film::put
 * following, line by line, the files listed in SURVEY.md §8(c).  Each function
 * cites the reference file:line (relative to /root/reference) it restates.
 *
 * PARITY STATUS — "parity unpinned" at two boundaries, pinned elsewhere:
 *   * The reference cannot be built in this image (Embree3, TBB, Eigen,
 *     pugixml, fmt, OpenImageIO are absent, nothing can be installed) and it
 *     ships no tests, fixtures or golden images.  The only leaf
 *     that compiles from its own sources, ext/rgb2spec, IS built (oracle/_ref)
 *     and pins rgb2spec_fetch below bit for bit.
 *   * Embree 3 (vcpkg.json:10, no version pinned): ray/triangle arithmetic and
 *     BVH visiting order live there.  intersect_triangle() restates Embree 3's
 *     published Moeller-Trumbore test (kernels/geometry/
 *     triangle_intersector_moeller.h: C = v0-O, R = C x D, den = Ng.D,
 *     U = R.e2, V = R.e1, T = Ng.C; accept den != 0, U,V >= 0, U+V <= |den|,
 *     |den| tnear < T <= |den| tfar; t,u,v = T,U,V / |den|) with an exact
 *     reciprocal in place of Embree's rcp+Newton step, and replaces the
 *     BVH-order-dependent tie rule by "smallest t, then smallest scene-global
 *     triangle index", which no traversal order can change.
 *   * Eigen (vcpkg.json:7, no version pinned): expression order, rule R2 of
 *     oracle_math.h.
 *   Everything else is pinned by the golden vectors of SURVEY §8(c)
 *   (tests/golden/), which tests/test_oracle_kat.py checks.
 *
 * Deliberate deviations from the reference as written:
 *   D1 (F6)  max_depth / rr_depth / hide_emitters default to the values the
 *            PathTracer's shadowing members hold (path.cpp:135-136): -1, 5, false.
 *   D2 (F7)  seeding: MSK_RNG_PCG_BLOCK = one PCG32 seeded
 *            (0x853c49e6748fea9b + base_seed, 0xda3e39cb94b95bdb) at the start
 *            of every block ("one block per TBB task"); MSK_RNG_COUNTER = a
 *            stateless hash of (seed, pixel, sample, dimension pair).
 *   D3 (F8)  bsdf->sample(ctx, si, next1d(), next2d()) draws left to right.
 *   D4       the two extra sample_ray() calls of sample_ray_differential
 *            (sensor.cpp:64,70) are skipped: their outputs are only read by
 *            BSDFs that need differentials (bsdf.cpp:18), none on this path.
 *   D5       Mesh::m_surface_area starts from 0 (the reference accumulates
 *            into an uninitialised float, mesh.h:93, mesh.cpp:44).
 *   D6       blocks are added to the film in spiral-id order (the reference
 *            adds them in arrival order under a mutex, hdrfilm.cpp:43-46).
 *   D7       transcendental functions: rule R3 of oracle_math.h.
 *   D8       ConstantBackgroundEmitter::sample_direct evaluates its radiance on a
 *            default-constructed interaction whose wavelengths are uninitialised
 *            (constant.cpp:68-71); the wavelengths of the reference point are
 *            used, as AreaLight::sample_direct does (area.cpp:35-36).
 *   D9       rough conductor / rough dielectric / twosided are not in the
 *            reference's build and need small repairs to compile
 *            (roughdielectric.cpp:67 multiplies an Eigen float vector by a double;
 *            Color3 weights become 4-wavelength spectra).  They are restated as
 *            written otherwise, including: only the GGX branches exist
 *            (microfacet.h:115-118,135-137 leave Beckmann empty); "sample_visible"
 *            changes the weight but still draws m from D(m)cos (microfacet.h:19-41);
 *            sample() omits specular_transmittance (roughdielectric.cpp:95-100);
 *            a BSDF sample that leaves the scene keeps the NEE record for its MIS
 *            weight (path.cpp:90-95,103-108).  These paths are pinned by closed-form
 *            properties (tests/test_rough_*.py, tests/test_environment.py), not by
 *            reference outputs: "parity unpinned" applies to them.
 *            The smooth `dielectric` (bsdfs/dielectric.cpp) is in the same position: left out of
 *            the reference's build (src/librender/CMakeLists.txt:63), its tints read through
 *            eval_3.  Restated as written with the same repair (the tints are spectra at the
 *            path's wavelengths); pinned by float64 (tests/test_dielectric_parity.py: Fresnel
 *            term, Snell's law, where a refracted ray lands), not by reference outputs.
 *   D10      ray/triangle acceptance = the Moeller-Trumbore test above AND "the hit point
 *            o + t d lies in the triangle's own bounding box (grown by 0.5e-5 of the scene's
 *            scale = max(diagonal, largest |coordinate|))": see intersect_triangle().  Found by the randomised parity sweep
 *            (tools/fuzz_parity.py): a shadow ray lying in the plane of a sliver emitter
 *            triangle produced a numerical "hit" 40 units outside the triangle that one
 *            tree reported and another culled.
 *   The features merged after the glass twin are restated from the text of include/msk_gpu.h (msk_texture_desc,
 *   msk_envmap_desc, msk_point_desc, MSK_BSDF_CONDUCTOR, msk_mask_desc) and from the tests' fp32 restatements (envmap_ref.py, delta_ref.py, bitmap_ref.py, mask_ref.py), not from the device's
 *   code; their departures from the reference as written are DESIGN.md section 9, (1)-(8):
 *   D11 (1)  envmap: a piecewise-constant distribution over the texels (per-row tables and a marginal, built in double and
 *            stored as float), not core/distribution.h's Distribution2D.
 *   D12 (2)  envmap hit by a BSDF sample: L(ray direction) and pdf(ray direction) / n_emitters, not path.cpp's stale records.
 *   D13 (3)  envmap and bitmap texels are spectra ({c0, c1, c2, w} / three coefficients); spectral VALUES are interpolated.
 *   D14 (4)  a point light's next-event term has weight 1, not mis_weight(1, bsdf_pdf).
 *   D15 (5)  in a scene that holds a point emitter, a `conductor` entry or a mask (the facts the launch plan reads) a
 *            `constant` sky hit by a BSDF sample counts with (1 / 4 pi) / n_emitters; every other scene keeps D9's stale record.
 *   D16 (6)  mask: the nested lobe has X's value and the density a pdf_X (mask.cpp multiplies the value AND keeps the pdf).
 *   D17 (7)  mask: the opacity is a scalar.
 *   D18 (8)  mask: under hide_emitters an AREA emitter reached while `scattered` is false adds nothing.
 *   `plastic` and `roughplastic` (types 6 and 7) are restated from the text of include/msk_gpu.h at msk_bsdf_desc (MSK_BSDF_PLASTIC,
 *   MSK_BSDF_ROUGHPLASTIC) and from the tests' fp32 restatements (plastic_ref.py, roughplastic_ref.py), not from the device's code; the
 *   reference's bsdfs/roughplastic.cpp is RGB-typed and not built, so the header's text is the specification:
 *   D19      plastic: the coat is a delta lobe that sets kDelta per SAMPLE while the entry keeps its smooth lobe: every hit takes its
 *            next-event sample (the diffuse lobe's eval / pdf alone), and an emitter or sky the mirrored ray reaches counts with
 *            emitter density 0, weight exactly 1.
 *   D20      the two constants fdr_int and ssw are computed here per entry, in double, by a rule of this file's own (plastic_fdr_int:
 *            24-point Gauss-Legendre on dyadic panels towards mu = 0, where the integrand's nearest singularity lies for eta near 1;
 *            the packer's is 64 points on four equal panels) and rounded once to fp32; csrc/msk_plastic_tables.h is not included.
 *   D21      roughplastic: no visible-normal variant.  The sample_visible word is read as `nonlinear` for both types; the normal is
 *            drawn from D(m) cos(theta_m) (sample_ggx) and the coat's density is (D H.z) / (4 dot(wo, H)), where roughplastic.cpp:144-146
 *            returns the visible-normal density under the flag (biased there: tests/test_roughplastic_bsdf.py).
 *   D22      a scene that holds a plastic of either type counts a `constant` sky with its own density (D15): it runs the kernels a
 *            mask scene runs.  The `direct` integrator refuses such a scene.
 *   D23      the next-event sample of the `spot` and `directional` emitters (msk_gpu.h at msk_light_desc; tests/light_ref.py), no more:
 *            two closed forms of each plastic are lit by a sun, and the twin has to render them.  Delta lights like the point light
 *            (D14: weight 1; D15: such a scene counts a `constant` sky with its own density); the refusals of msk_light_desc; a
 *            scene whose spot or sun comes without its descriptor, or an emitter type this file does not know, is refused where it
 *            ran the area light's code before.  Their tallies (spot_beam / _ramp / _dark, spot_ / sun_occluded / _unoccluded, and the
 *            direct integrator's light_spot_* / light_sun_*) tell the falloff's three branches and the three delta lights apart.
 *   D24      the `thinlens` sensor, written from the six steps at msk_lens_desc in msk_gpu.h (tests/lens_ref.py is the second witness),
 *            not from the device's code: near_p as the pinhole computes it; the lens point from this file's own
 *            square_to_uniform_disk_concentric times R; the focus point near_p (f / near_p.z); the direction normalized in camera
 *            space, tnear / tfar from its z; origin and direction through apply_point / apply_vector.  The aperture sample is pair 2 of
 *            the sample's key under MSK_RNG_COUNTER and no other draw moves; R = 0 goes through this code; a scene without a lens keeps
 *            camera_ray as it was.  Every render entry point refuses a lens scene under MSK_RNG_PCG_BLOCK (the library:
 *            MSK_ERR_UNSUPPORTED); scene creation refuses what msk_lens_desc lists.  A scene with a lens counts a `constant` sky
 *            with its own density (D15), whatever else it holds: msk_lens_desc gives it kernels of its own that carry the mask code,
 *            and msk_mask_desc says "A `constant` sky counts with the density of the ray's own direction, as in every scene that
 *            runs the kernels of msk_point_desc" (D22 reads the plastics the same way).  Found by the randomised sweep: the twin
 *            kept D9's stale record for a lens over a `constant` sky and nothing else, and every such scene's film differed.
 */
#include "oracle_math.h"
#include "msk_gpu.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

namespace orc {

int g_use_libm = 0;
int g_trace_path = 0;     // debugging aid: print the per-bounce state of path_sample (msk_oracle_set_trace)

// ===========================================================================
// scene data derived from the flattened description
// ===========================================================================
struct Tri { V3 p0, p1, p2; };

struct BVHNode {            // oracle's own accelerator, not the GPU's layout
    V3 lo, hi;
    int left, right;        // inner: children; leaf: left = -1
    int first, count;       // leaf: range in tri_order
};

struct Scene {
    std::vector<msk_mesh_desc> meshes;
    std::vector<msk_bsdf_desc> bsdfs;
    std::vector<msk_emitter_desc> emitters;
    std::vector<msk_texture_desc> textures;
    std::vector<float> vertices;
    std::vector<uint32_t> faces;
    msk_camera_desc camera;
    msk_film_desc film;
    float cie[3 * MSK_CIE_SAMPLES];
    float d65[MSK_CIE_SAMPLES];

    std::vector<Tri> tris;                 // scene-global triangle list
    std::vector<uint32_t> tri_mesh;        // global triangle -> mesh index
    std::vector<float> mesh_area;          // Mesh::m_surface_area
    std::vector<std::vector<float>> mesh_cdf;  // Distribution1D::m_cdf per mesh
    std::vector<std::vector<float>> emitter_d65;  // RegularSpectrum::m_pdf per emitter
    // spectra/regular.cpp:27-70: RegularSpectrum::m_distr of every tabulated spectrum of the scene (ABI v7), and which grid the
    // emitter's radiance table lives on (the D65 grid, or its own when the radiance is a `regular` spectrum)
    struct RegularTable { float range_x, inv_interval; std::vector<float> pdf; };
    std::vector<RegularTable> regular;
    std::vector<RegularTable> emitter_table;
    float tri_pad = 0.f;                   // D10: half the BVH padding, see intersect_triangle
    int env = -1;                          // Scene::m_environment as an index into emitters
    float env_radius = 0.f;                // ConstantBackgroundEmitter::m_bsphere.radius after set_scene
    std::vector<float> texels;             // msk_scene_desc.texels: 3 coefficients per texel (bitmap textures)
    // msk_envmap_desc: the image, its rotation and the tables built from the host's weights (cumulative(), in double stored as float)
    struct Envmap { uint32_t W = 0, H = 0; std::vector<float> texels, marg; std::vector<std::vector<float>> cond; float R[9]; };
    Envmap envmap;
    bool env_is_image = false;
    std::vector<V3> point_pos;             // msk_point_desc.position per emitter (MSK_EMITTER_POINT entries only)
    // msk_light_desc per emitter (MSK_EMITTER_SPOT / MSK_EMITTER_DIRECTIONAL entries only; D23)
    struct Light { V3 position, direction; float cos_cutoff = 0.f, cos_beam = 0.f; };
    std::vector<Light> lights;
    bool any_sun = false;
    // msk_mask_desc per BSDF entry (filter < 0: the entry has no mask)
    struct Mask { int filter = -1; float opacity = 1.f; float to_uv[6]; uint32_t W = 0, H = 0; std::vector<float> values; };
    std::vector<Mask> masks;
    bool any_mask = false;
    bool own_density_sky = false;          // D15: a point emitter, a `conductor` entry, a mask or a plastic (D22) is in the scene, or it has a lens (D24)
    // D20: {fdr_int, ssw} per BSDF entry ({0, 0} for an entry that is no plastic)
    struct PlasticK { float fdr_int = 0.f, ssw = 0.f; };
    std::vector<PlasticK> plastic_k;
    bool any_plastic = false;
    // msk_lens_desc (D24); has_lens false: the pinhole camera of msk_camera_desc alone
    bool has_lens = false;
    float lens_radius = 0.f, lens_focus = 0.f;

    std::vector<BVHNode> nodes;
    std::vector<uint32_t> tri_order;
    int use_bvh = 1;

    const float *vertex(uint32_t mesh, uint32_t local_index) const {   // mesh.h:21-26
        return &vertices[(size_t) (meshes[mesh].first_vertex + local_index) * 8];
    }
    const uint32_t *face(uint32_t mesh, uint32_t local_face) const {   // mesh.h:28-33
        return &faces[(size_t) (meshes[mesh].first_face + local_face) * 3];
    }
    V3 vertex_position(uint32_t mesh, uint32_t i) const {              // mesh.h:39-42
        const float *v = vertex(mesh, i); return mk3(v[0], v[1], v[2]);
    }
    V3 vertex_normal(uint32_t mesh, uint32_t i) const {                // mesh.h:44-47
        const float *v = vertex(mesh, i) + 3; return mk3(v[0], v[1], v[2]);
    }
    V2 vertex_texcoord(uint32_t mesh, uint32_t i) const {              // mesh.h:49-52
        const float *v = vertex(mesh, i) + 6; return V2{v[0], v[1]};
    }
};

// mesh.h:54-61  face_area
static float face_area(const Scene &sc, uint32_t mesh, uint32_t f) {
    const uint32_t *fi = sc.face(mesh, f);
    V3 p0 = sc.vertex_position(mesh, fi[0]), p1 = sc.vertex_position(mesh, fi[1]),
       p2 = sc.vertex_position(mesh, fi[2]);
    return 0.5f * norm(cross(p1 - p0, p2 - p0));
}

// mesh.cpp:39-48 area_distr_build + core/distribution.h:88-96 Distribution1D::init
static void area_distr_build(Scene &sc, uint32_t mesh) {
    float surface_area = 0.f;                                    // D5
    std::vector<float> cdf;
    cdf.push_back(0.f);
    float run = 0.f;
    bool first = true;
    for (uint32_t i = 0; i < sc.meshes[mesh].face_count; ++i) {
        float a = face_area(sc, mesh, i);
        surface_area += a;
        run = first ? a : run + a;                               // std::partial_sum
        first = false;
        cdf.push_back(run);
    }
    const float inv_sum = 1.f / cdf.back();
    for (auto &c : cdf) c *= inv_sum;
    sc.mesh_area[mesh] = surface_area;
    sc.mesh_cdf[mesh] = cdf;
}

// ---------------------------------------------------------------------------
// oracle BVH: median split, leaves <= 4 triangles, boxes padded so that the
// slab test can never cull a triangle intersect_triangle() would accept.
// ---------------------------------------------------------------------------
static void tri_bounds(const Tri &t, V3 *lo, V3 *hi) {
    lo->x = std::min(t.p0.x, std::min(t.p1.x, t.p2.x)); hi->x = std::max(t.p0.x, std::max(t.p1.x, t.p2.x));
    lo->y = std::min(t.p0.y, std::min(t.p1.y, t.p2.y)); hi->y = std::max(t.p0.y, std::max(t.p1.y, t.p2.y));
    lo->z = std::min(t.p0.z, std::min(t.p1.z, t.p2.z)); hi->z = std::max(t.p0.z, std::max(t.p1.z, t.p2.z));
}
static int build_node(Scene &sc, int first, int count, float pad) {
    BVHNode nd;
    nd.lo = mk3(kInf, kInf, kInf); nd.hi = mk3(-kInf, -kInf, -kInf);
    V3 clo = nd.lo, chi = nd.hi;
    for (int i = first; i < first + count; ++i) {
        V3 lo, hi; tri_bounds(sc.tris[sc.tri_order[i]], &lo, &hi);
        nd.lo = mk3(std::min(nd.lo.x, lo.x), std::min(nd.lo.y, lo.y), std::min(nd.lo.z, lo.z));
        nd.hi = mk3(std::max(nd.hi.x, hi.x), std::max(nd.hi.y, hi.y), std::max(nd.hi.z, hi.z));
        V3 c = (lo + hi) * 0.5f;
        clo = mk3(std::min(clo.x, c.x), std::min(clo.y, c.y), std::min(clo.z, c.z));
        chi = mk3(std::max(chi.x, c.x), std::max(chi.y, c.y), std::max(chi.z, c.z));
    }
    nd.lo = nd.lo - mk3(pad, pad, pad); nd.hi = nd.hi + mk3(pad, pad, pad);
    nd.left = nd.right = -1; nd.first = first; nd.count = count;
    int idx = (int) sc.nodes.size();
    sc.nodes.push_back(nd);
    if (count <= 4) return idx;
    V3 ext = chi - clo;
    int axis = (ext.x >= ext.y && ext.x >= ext.z) ? 0 : (ext.y >= ext.z ? 1 : 2);
    auto key = [&](uint32_t t) {
        V3 lo, hi; tri_bounds(sc.tris[t], &lo, &hi);
        return axis == 0 ? lo.x + hi.x : axis == 1 ? lo.y + hi.y : lo.z + hi.z;
    };
    int mid = first + count / 2;
    std::nth_element(sc.tri_order.begin() + first, sc.tri_order.begin() + mid,
                     sc.tri_order.begin() + first + count,
                     [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    int l = build_node(sc, first, mid - first, pad);
    int r = build_node(sc, mid, first + count - mid, pad);
    sc.nodes[idx].left = l; sc.nodes[idx].right = r;
    return idx;
}

// msk_gpu.h at msk_envmap_desc: "The library builds, in double and stored as float, ... a cumulative table": entry k = the sum of
// the first k weights over the total, the last entry 1; a row of zero weight is 0 .. 0 1 (tests/envmap_ref.py: cumulative)
static std::vector<float> cumulative(const std::vector<double> &w) {
    std::vector<float> out(w.size() + 1, 0.f);
    double total = 0.0;
    for (double x : w) total += x;
    if (total > 0.0) { double run = 0.0; for (size_t k = 0; k < w.size(); ++k) { run += w[k]; out[k + 1] = (float) (run / total); } }
    out[w.size()] = 1.f;
    return out;
}
// msk_gpu.h: "must be a rotation: |R R^T - 1| <= 1e-4 per entry and det > 0, anything else is refused"
static bool is_rotation(const float *r) {
    for (int i = 0; i < 9; ++i) if (!std::isfinite(r[i])) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += (double) r[i * 3 + k] * (double) r[j * 3 + k];
            if (std::fabs(s - (i == j ? 1.0 : 0.0)) > 1e-4) return false;
        }
    const double det = (double) r[0] * ((double) r[4] * r[8] - (double) r[5] * r[7]) - (double) r[1] * ((double) r[3] * r[8] - (double) r[5] * r[6]) +
                       (double) r[2] * ((double) r[3] * r[7] - (double) r[4] * r[6]);
    return det > 0.0;
}
// ---------------------------------------------------------------------------
// D20: the two constants of a `plastic` / `roughplastic` entry (msk_gpu.h at msk_bsdf_desc), in double, rounded once by the caller
// ---------------------------------------------------------------------------
// the exact unpolarised Fresnel reflectance of a dielectric boundary met from the thin side at cosine mu, relative index eta >= 1
static double plastic_fresnel_exact(double mu, double eta) {
    if (eta == 1.0) return 0.0;
    const double sin2_t = (1.0 - mu * mu) / (eta * eta);              // Snell
    const double cos_t = std::sqrt(1.0 - sin2_t);                      // eta >= 1: no total reflection from this side
    const double rs = (mu - eta * cos_t) / (mu + eta * cos_t), rp = (eta * mu - cos_t) / (eta * mu + cos_t);
    return 0.5 * (rs * rs + rp * rp);
}
// fdr_int = 1 - (1 - fdr_ext) / eta^2 with fdr_ext = 2 int_0^1 F(mu) mu dmu.  F is analytic on (0, 1] with branch points at
// mu = +- i sqrt(eta^2 - 1), which approach mu = 0 as eta -> 1: the panels are [2^-(k+1), 2^-k], k = 0 .. 59, so that every panel
// keeps the branch points at least its own length away (a 24-point rule then converges past 1e-16 per panel); what is left,
// [0, 2^-60], holds less than 2^-120.
static double plastic_fdr_int(double eta) {
    if (eta == 1.0) return 0.0;
    constexpr int N = 24;
    static double node[N], weight[N];
    static std::once_flag once;
    std::call_once(once, [] {
        const double pi = 3.14159265358979323846;
        for (int i = 0; i < N; ++i) {                                  // the roots of the Legendre polynomial P_24 by Newton's iteration
            double x = std::cos(pi * (i + 0.75) / (N + 0.5)), d = 1.0;
            for (int it = 0; it < 64; ++it) {
                double a = 1.0, b = x;
                for (int k = 2; k <= N; ++k) { const double c = ((2 * k - 1) * x * b - (k - 1) * a) / k; a = b; b = c; }
                d = N * (a - x * b) / (1.0 - x * x);
                const double step = b / d;
                x -= step;
                if (std::fabs(step) < 1e-17) break;
            }
            double a = 1.0, b = x;
            for (int k = 2; k <= N; ++k) { const double c = ((2 * k - 1) * x * b - (k - 1) * a) / k; a = b; b = c; }
            d = N * (a - x * b) / (1.0 - x * x);
            node[i] = x; weight[i] = 2.0 / ((1.0 - x * x) * d * d);
        }
    });
    double total = 0.0;
    for (int k = 59; k >= 0; --k) {                                    // the small panels first
        const double lo = std::ldexp(1.0, -(k + 1)), half = 0.5 * lo;  // [lo, 2 lo]
        double panel = 0.0;
        for (int i = 0; i < N; ++i) {
            const double mu = lo + half * (node[i] + 1.0);
            panel += weight[i] * plastic_fresnel_exact(mu, eta) * mu;
        }
        total += half * panel;
    }
    return 1.0 - (1.0 - 2.0 * total) / (eta * eta);
}
// the sigmoid polynomial S(coeff, l) of render/srgb.h:8-19 in double ({0, 0, +-inf}: the constants 1 and 0)
static double plastic_sigmoid(const float *c, double l) {
    if (std::isinf(c[2])) return c[2] > 0.f ? 1.0 : 0.0;
    const double x = ((double) c[0] * l + (double) c[1]) * l + (double) c[2];
    return std::max(0.5 + x / (2.0 * std::sqrt(1.0 + x * x)), 0.0);
}
static double plastic_mean_sigmoid(const float *c) {
    double s = 0.0;
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) s += plastic_sigmoid(c, 360.0 + 5.0 * i);
    return s / MSK_CIE_SAMPLES;
}
// the mean over the 95 CIE wavelengths of the tabulated spectrum k (1-based; msk_regular_spectrum_desc: lerp, the end segments continued)
static double plastic_mean_regular(const msk_scene_desc *d, uint32_t k) {
    const msk_regular_spectrum_desc &r = d->regular_spectra[k - 1];
    const double step = ((double) r.lambda_max - (double) r.lambda_min) / (double) (r.size - 1);
    const float *v = d->regular_values + r.first_value;
    double s = 0.0;
    for (int i = 0; i < MSK_CIE_SAMPLES; ++i) {
        const double x = (360.0 + 5.0 * i - (double) r.lambda_min) / step;
        const long seg = std::min(std::max((long) std::floor(x), 0l), (long) r.size - 2);
        const double t = x - (double) seg;
        s += (1.0 - t) * (double) v[seg] + t * (double) v[seg + 1];
    }
    return s / MSK_CIE_SAMPLES;
}
static void plastic_constants(const msk_scene_desc *d, const msk_bsdf_desc &b, double *fdr_int, double *ssw) {
    *fdr_int = plastic_fdr_int((double) b.ior_eta);
    const msk_spectrum_desc &sp = b.specular_reflectance;
    const double s_mean = sp.regular ? plastic_mean_regular(d, sp.regular) : (double) sp.scale * plastic_mean_sigmoid(sp.coeff);
    double d_mean;
    if (b.reflectance_regular) d_mean = plastic_mean_regular(d, b.reflectance_regular);
    else if (!b.reflectance_texture) d_mean = (double) b.reflectance_scale * plastic_mean_sigmoid(b.reflectance);
    else {
        const msk_texture_desc &t = d->textures[b.reflectance_texture - 1];
        if (t.type == MSK_TEXTURE_CHECKERBOARD) d_mean = 0.5 * (plastic_mean_sigmoid(t.color0) + plastic_mean_sigmoid(t.color1));
        else {
            const size_t n = (size_t) t.width * t.height;
            d_mean = 0.0;
            for (size_t k = 0; k < n; ++k) d_mean += plastic_mean_sigmoid(d->texels + ((size_t) t.first_texel + k) * 3);
            d_mean /= (double) n;
        }
    }
    *ssw = (d_mean + s_mean) > 0.0 ? s_mean / (d_mean + s_mean) : 1.0;
}
// What the library refuses of the BSDF entries at scene creation that this file would otherwise misread (msk_gpu.h at msk_bsdf_desc):
// an unassigned type, a back_bsdf out of range, and a plastic's ior_eta below 1, specular scale or roughness
static bool bsdfs_acceptable(const msk_scene_desc *d) {
    for (uint32_t i = 0; i < d->n_bsdfs; ++i) {
        const msk_bsdf_desc &b = d->bsdfs[i];
        const bool known = b.type == MSK_BSDF_DIFFUSE || b.type == MSK_BSDF_ROUGHCONDUCTOR || b.type == MSK_BSDF_ROUGHDIELECTRIC || b.type == MSK_BSDF_DIELECTRIC ||
                           b.type == MSK_BSDF_CONDUCTOR || b.type == MSK_BSDF_PLASTIC || b.type == MSK_BSDF_ROUGHPLASTIC;
        if (!known) return false;                                      // type 5, and 8 or more
        if (b.back_bsdf < -1 || b.back_bsdf >= (int32_t) d->n_bsdfs) return false;
        if (b.type == MSK_BSDF_PLASTIC || b.type == MSK_BSDF_ROUGHPLASTIC) {
            if (!(std::isfinite(b.ior_eta) && b.ior_eta >= 1.f)) return false;
            if (!(std::isfinite(b.ior_inv_eta) && b.ior_inv_eta > 0.f)) return false;
            if (b.specular_reflectance.regular == 0 && !std::isfinite(b.specular_reflectance.scale)) return false;
            if (b.specular_reflectance.regular > d->n_regular_spectra || b.reflectance_regular > d->n_regular_spectra || b.reflectance_texture > d->n_textures) return false;
        }
        if (b.type == MSK_BSDF_ROUGHPLASTIC) {
            if (!(std::isfinite(b.alpha_u) && std::isfinite(b.alpha_v) && b.alpha_u >= 0.f && b.alpha_v >= 0.f)) return false;
            if (b.alpha_u != b.alpha_v) return false;                  // roughplastic.cpp:23-25: no anisotropic coat
        }
    }
    return true;
}

// What a scene holds beyond msk_scene_desc; false = something the library refuses at scene creation (msk_gpu.h at
// msk_gpu_scene_create_env / _ext / _masks)
static bool scene_extensions(Scene *sc, const msk_scene_desc *d, const msk_scene_masks *em, uint32_t n_lights, const msk_light_desc *lights) {
    const msk_envmap_desc *env = em ? em->ext.envmap : nullptr;
    uint32_t n_env = 0, n_image = 0;
    for (uint32_t e = 0; e < d->n_emitters; ++e) {
        const int32_t t = d->emitters[e].type;
        if (t == MSK_EMITTER_CONSTANT || t == MSK_EMITTER_ENVMAP) ++n_env;
        if (t == MSK_EMITTER_ENVMAP) ++n_image;
        if ((t == MSK_EMITTER_POINT || t == MSK_EMITTER_SPOT || t == MSK_EMITTER_DIRECTIONAL) && d->emitters[e].mesh_id != -1) return false;
        if (t < MSK_EMITTER_AREA || t > MSK_EMITTER_DIRECTIONAL) return false;      // no unknown emitter type reaches the area light's code
    }
    if (n_env > 1 || (n_image != 0) != (env != nullptr)) return false;
    if (env) {
        if (env->width == 0 || env->height == 0 || !env->texels || !env->weights || !is_rotation(env->to_world)) return false;
        Scene::Envmap &m = sc->envmap;
        m.W = env->width; m.H = env->height;
        const size_t n = (size_t) m.W * m.H;
        m.texels.assign(env->texels, env->texels + n * 4);
        std::memcpy(m.R, env->to_world, sizeof(m.R));
        bool any = false;
        for (size_t k = 0; k < n; ++k) {
            if (!(std::isfinite(env->weights[k]) && env->weights[k] >= 0.f) || !(std::isfinite(m.texels[k * 4 + 3]) && m.texels[k * 4 + 3] >= 0.f)) return false;
            any |= env->weights[k] > 0.f;
        }
        if (!any) return false;
        std::vector<double> rows(m.H), row(m.W);
        m.cond.resize(m.H);
        for (uint32_t j = 0; j < m.H; ++j) {
            double sum = 0.0;
            for (uint32_t i = 0; i < m.W; ++i) { row[i] = (double) env->weights[(size_t) j * m.W + i]; sum += row[i]; }      // (row sums added left to right)
            rows[j] = sum;
            m.cond[j] = cumulative(row);
        }
        m.marg = cumulative(rows);
        sc->env_is_image = true;
    }
    // exactly one msk_point_desc per MSK_EMITTER_POINT emitter, in any order
    sc->point_pos.assign(d->n_emitters, mk3(0.f, 0.f, 0.f));
    std::vector<int> seen(d->n_emitters, 0);
    const uint32_t n_points = em ? em->ext.n_points : 0u;
    for (uint32_t k = 0; k < n_points; ++k) {
        const msk_point_desc &p = em->ext.points[k];
        if (p.emitter >= d->n_emitters || d->emitters[p.emitter].type != MSK_EMITTER_POINT || seen[p.emitter]++) return false;
        if (!(std::isfinite(p.position[0]) && std::isfinite(p.position[1]) && std::isfinite(p.position[2]))) return false;
        sc->point_pos[p.emitter] = mk3(p.position[0], p.position[1], p.position[2]);
    }
    bool any_point = false;
    for (uint32_t e = 0; e < d->n_emitters; ++e)
        if (d->emitters[e].type == MSK_EMITTER_POINT) { any_point = true; if (!seen[e]) return false; }
    // D23: exactly one msk_light_desc per MSK_EMITTER_SPOT / MSK_EMITTER_DIRECTIONAL emitter, in any order (the refusals listed at msk_light_desc)
    sc->lights.assign(d->n_emitters, Scene::Light());
    std::vector<int> lit(d->n_emitters, 0);
    if (n_lights && !lights) return false;
    bool any_light = false;
    for (uint32_t k = 0; k < n_lights; ++k) {
        const msk_light_desc &l = lights[k];
        if (l.emitter >= d->n_emitters || lit[l.emitter]++) return false;
        const int32_t t = d->emitters[l.emitter].type;
        if (t != MSK_EMITTER_SPOT && t != MSK_EMITTER_DIRECTIONAL) return false;
        const double n2 = (double) l.direction[0] * l.direction[0] + (double) l.direction[1] * l.direction[1] + (double) l.direction[2] * l.direction[2];
        if (!(std::isfinite(l.direction[0]) && std::isfinite(l.direction[1]) && std::isfinite(l.direction[2])) || !(std::fabs(n2 - 1.0) <= 1e-5)) return false;
        if (t == MSK_EMITTER_SPOT) {
            if (!(std::isfinite(l.position[0]) && std::isfinite(l.position[1]) && std::isfinite(l.position[2]))) return false;
            if (!(l.cos_cutoff >= -1.f && l.cos_cutoff < 1.f) || !(l.cos_beam >= l.cos_cutoff && l.cos_beam <= 1.f)) return false;
        }
        Scene::Light &o = sc->lights[l.emitter];
        o.position = mk3(l.position[0], l.position[1], l.position[2]); o.direction = mk3(l.direction[0], l.direction[1], l.direction[2]);
        o.cos_cutoff = l.cos_cutoff; o.cos_beam = l.cos_beam;
    }
    for (uint32_t e = 0; e < d->n_emitters; ++e) {
        const int32_t t = d->emitters[e].type;
        if (t == MSK_EMITTER_SPOT || t == MSK_EMITTER_DIRECTIONAL) { any_light = true; if (!lit[e]) return false; }
        if (t == MSK_EMITTER_DIRECTIONAL) sc->any_sun = true;
    }
    // at most one msk_mask_desc per entry
    sc->masks.assign(d->n_bsdfs, Scene::Mask());
    const uint32_t n_masks = em ? em->n_masks : 0u;
    for (uint32_t k = 0; k < n_masks; ++k) {
        const msk_mask_desc &md = em->masks[k];
        if (md.bsdf >= d->n_bsdfs || sc->masks[md.bsdf].filter >= 0 || md.filter < 0 || md.filter > 2) return false;
        Scene::Mask &m = sc->masks[md.bsdf];
        m.filter = md.filter; m.opacity = md.opacity;
        std::memcpy(m.to_uv, md.to_uv, sizeof(m.to_uv));
        if (md.filter == 0) {
            if (!(std::isfinite(md.opacity) && md.opacity >= 0.f && md.opacity <= 1.f)) return false;
        } else {
            if (md.width == 0 || md.height == 0 || !md.values) return false;
            m.W = md.width; m.H = md.height;
            m.values.assign(md.values, md.values + (size_t) m.W * m.H);
            for (float v : m.values) if (!(std::isfinite(v) && v >= 0.f && v <= 1.f)) return false;
        }
        sc->any_mask = true;
    }
    bool any_conductor = false;
    for (uint32_t b = 0; b < d->n_bsdfs; ++b) any_conductor |= d->bsdfs[b].type == MSK_BSDF_CONDUCTOR;
    // D20: the constants of the plastics, each rounded once
    sc->plastic_k.assign(d->n_bsdfs, Scene::PlasticK());
    for (uint32_t b = 0; b < d->n_bsdfs; ++b)
        if (d->bsdfs[b].type == MSK_BSDF_PLASTIC || d->bsdfs[b].type == MSK_BSDF_ROUGHPLASTIC) {
            double fdr_int, ssw;
            plastic_constants(d, d->bsdfs[b], &fdr_int, &ssw);
            sc->plastic_k[b].fdr_int = (float) fdr_int; sc->plastic_k[b].ssw = (float) ssw;
            sc->any_plastic = true;
        }
    sc->own_density_sky = any_point || any_light || any_conductor || sc->any_mask || sc->any_plastic;      // D15, D22, D23
    return true;
}

static Scene *scene_from_desc(const msk_scene_desc *d, const msk_scene_masks *em = nullptr, uint32_t n_lights = 0, const msk_light_desc *lights = nullptr,
                              const msk_lens_desc *lens = nullptr) {
    if (!bsdfs_acceptable(d)) return nullptr;
    // msk_lens_desc: "aperture_radius negative, NaN or infinite; focus_distance not finite or not greater than 0"
    if (lens && (!(std::isfinite(lens->aperture_radius) && lens->aperture_radius >= 0.f) || !(std::isfinite(lens->focus_distance) && lens->focus_distance > 0.f))) return nullptr;
    Scene *sc = new Scene();
    if (lens) { sc->has_lens = true; sc->lens_radius = lens->aperture_radius; sc->lens_focus = lens->focus_distance; }
    if (!scene_extensions(sc, d, em, n_lights, lights)) { delete sc; return nullptr; }
    if (sc->has_lens) sc->own_density_sky = true;                  // D24: the lens' kernels carry the mask code and its sky rule
    if (d->n_texels) sc->texels.assign(d->texels, d->texels + (size_t) d->n_texels * 3);
    sc->meshes.assign(d->meshes, d->meshes + d->n_meshes);
    sc->bsdfs.assign(d->bsdfs, d->bsdfs + d->n_bsdfs);
    sc->emitters.assign(d->emitters, d->emitters + d->n_emitters);
    if (d->n_textures) sc->textures.assign(d->textures, d->textures + d->n_textures);
    sc->vertices.assign(d->vertices, d->vertices + (size_t) d->n_vertices * 8);
    sc->faces.assign(d->faces, d->faces + (size_t) d->n_faces * 3);
    sc->camera = d->camera;
    sc->film = d->film;
    std::memcpy(sc->cie, d->cie1931_xyz, sizeof(sc->cie));
    std::memcpy(sc->d65, d->d65, sizeof(sc->d65));
    sc->tris.resize(d->n_faces);
    sc->tri_mesh.resize(d->n_faces);
    sc->mesh_area.resize(d->n_meshes);
    sc->mesh_cdf.resize(d->n_meshes);
    for (uint32_t m = 0; m < d->n_meshes; ++m) {
        const msk_mesh_desc &md = sc->meshes[m];
        for (uint32_t f = 0; f < md.face_count; ++f) {
            const uint32_t *fi = sc->face(m, f);
            Tri t{sc->vertex_position(m, fi[0]), sc->vertex_position(m, fi[1]),
                  sc->vertex_position(m, fi[2])};
            sc->tris[md.first_face + f] = t;
            sc->tri_mesh[md.first_face + f] = m;
        }
        area_distr_build(*sc, m);
    }
    // spectra/regular.cpp:27-70: SpectrumContinuousDistribution(range, values, size); update() computes the interval in double
    // and keeps 1 / interval as a float (:66-70)
    for (uint32_t k = 0; k < d->n_regular_spectra; ++k) {
        const msk_regular_spectrum_desc &r = d->regular_spectra[k];
        Scene::RegularTable t;
        t.range_x = r.lambda_min;
        const double interval_size = ((double) r.lambda_max - (double) r.lambda_min) / (double) (r.size - 1);
        t.inv_interval = (float) (1.0 / interval_size);
        t.pdf.assign(d->regular_values + r.first_value, d->regular_values + r.first_value + r.size);
        sc->regular.push_back(t);
    }
    // spectra/srgb_d65.cpp:24-31 -> d65.cpp:37-45: values = d65_data[i] * m_scale
    sc->emitter_d65.resize(d->n_emitters);
    sc->emitter_table.resize(d->n_emitters);
    for (uint32_t e = 0; e < d->n_emitters; ++e) {
        sc->emitter_d65[e].resize(MSK_CIE_SAMPLES);
        for (int i = 0; i < MSK_CIE_SAMPLES; ++i)
            sc->emitter_d65[e][i] = sc->d65[i] * sc->emitters[e].d65_scale;
        if (sc->emitters[e].radiance_regular) sc->emitter_table[e] = sc->regular[sc->emitters[e].radiance_regular - 1];
        else sc->emitter_table[e] = Scene::RegularTable{360.f, (float) (1.0 / ((830.0 - 360.0) / 94.0)), sc->emitter_d65[e]};
    }
    // scene.cpp:35-41 m_environment; constant.cpp:21-28 set_scene: sphere around Scene::bbox() (bbox.h:105-112)
    for (uint32_t e = 0; e < d->n_emitters; ++e)
        if (sc->emitters[e].type == MSK_EMITTER_CONSTANT || sc->emitters[e].type == MSK_EMITTER_ENVMAP) sc->env = (int) e;
    if (sc->env >= 0 || sc->any_sun) {                             // (msk_light_desc: a scene with a sun computes it whether it holds an environment emitter or not)
        V3 pmin = mk3(kInf, kInf, kInf), pmax = mk3(-kInf, -kInf, -kInf);
        for (uint32_t v = 0; v < d->n_vertices; ++v) {
            const float *q = &sc->vertices[(size_t) v * 8];
            pmin = mk3(std::min(pmin.x, q[0]), std::min(pmin.y, q[1]), std::min(pmin.z, q[2]));
            pmax = mk3(std::max(pmax.x, q[0]), std::max(pmax.y, q[1]), std::max(pmax.z, q[2]));
        }
        V3 c = (pmin + pmax) * .5f, r = c - pmax;
        float radius = std::sqrt(squared_norm(r));
        sc->env_radius = std::max(kRayEpsilon, radius * (1.f + kRayEpsilon));
    }
    // BVH
    sc->tri_order.resize(d->n_faces);
    for (uint32_t i = 0; i < d->n_faces; ++i) sc->tri_order[i] = i;
    V3 lo = mk3(kInf, kInf, kInf), hi = mk3(-kInf, -kInf, -kInf);
    for (auto &t : sc->tris) {
        V3 a, b; tri_bounds(t, &a, &b);
        lo = mk3(std::min(lo.x, a.x), std::min(lo.y, a.y), std::min(lo.z, a.z));
        hi = mk3(std::max(hi.x, b.x), std::max(hi.y, b.y), std::max(hi.z, b.z));
    }
    // D10 / node padding: 0.5e-5 (triangle bounds) and 1e-5 (node boxes) of the scene's SCALE = the larger of its diagonal and
    // its largest coordinate magnitude — what the rounding errors of the hit point and of the slab tests are proportional to
    // (a scene far from the origin has the ulps of its coordinates, not of its extent)
    float diag = d->n_faces ? norm(hi - lo) : 1.f;
    float amax = 0.f;
    if (d->n_faces) amax = std::max(std::max(std::max(std::fabs(lo.x), std::fabs(hi.x)), std::max(std::fabs(lo.y), std::fabs(hi.y))), std::max(std::fabs(lo.z), std::fabs(hi.z)));
    // (MSK_PAD_SCALE, read by the GPU library too: tests/test_padding_margin.py and test_fuzz_parity.py shrink the padding to show
    // how far the rule is from failing)
    const float pad_scale = getenv("MSK_PAD_SCALE") ? (float) atof(getenv("MSK_PAD_SCALE")) : 1e-5f;
    sc->tri_pad = (0.5f * pad_scale) * std::max(diag, amax);       // the nodes' padding (twice this) strictly contains it
    if (d->n_faces) build_node(*sc, 0, (int) d->n_faces, 2.f * sc->tri_pad);
    return sc;
}

// ===========================================================================
// a6/a7  Scene::ray_intersect / ray_test (scene.cpp:216-273) — Embree restated
// ===========================================================================
struct Ray { V3 o, d; float mint, maxt; };
struct Hit { float t, u, v; uint32_t prim; bool valid; };

// How far the two oracle-side rules are from a plain Moeller-Trumbore / first-found intersector: per-thread
// tallies, summed into g_isect by isect_flush() (the render workers and the ray batches call it through tallies_flush()), read and cleared through
// msk_oracle_isect_counters().  [0] closest-hit rays  [1] any-hit rays  [2] triangle tests Moeller-Trumbore accepts
// [3] of those, rejected by the D10 bounds predicate  [4] closest-hit rays that met a D10-rejected hit NEARER than the hit
// they report (or report none): the rays whose answer D10 can have changed, as this tree's traversal meets them
// [5] any-hit rays reported unoccluded that met a D10-rejected hit  [6] closest-hit rays whose reported t is shared by
// a second triangle (the "smallest prim" rule decided)  [7] accepted-hit pairs with equal t met on the way
static std::atomic<uint64_t> g_isect[8];
struct IsectTally { uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; float rej_t = kInf; bool rej = false; };
static thread_local IsectTally tl_isect;
static void isect_flush() { for (int i = 0; i < 8; ++i) { g_isect[i].fetch_add(tl_isect.v[i], std::memory_order_relaxed); tl_isect.v[i] = 0; } }

// Named path events (msk_oracle_path_tallies, read and clear like the intersection tallies): which branches of the path loop a
// render reached, so that a parity scene can be shown to exercise what it is meant to exercise.
enum PathTally { kTallyNullLobe, kTallyEmitterAfterNull, kTallyEmitterAfterDelta, kTallyEnvmapMissSmooth, kTallyPointUnoccluded, kTallyPointOccluded,
                 kTallySkyOwnDensity, kTallyAreaHidden, kTallyRRAfterNull, kTallyTexelWrap, kTallyPoleClamp,
                 kTallyShadowNonzero,      // next-event samples whose unoccluded term is not zero: the shadow rays the device traces
                 kTallyDeadSample,         // BSDF samples that failed or left a zero throughput: where the device's segment count may differ by one
                 kTallySegmentDropped,     // a sample with a lobe whose throughput is zero and no shadow ray pending: the wavefront kernels end the path, no ray
                 kTallySegmentExtra,       // a failed sample with a shadow ray pending: the wavefront kernels keep the slot one more sweep, one (zero) ray
                 // the plastics' branches (D19-D22), appended so that the eleven named events and the four counter tallies above keep their places
                 kTallyPlasticCoat, kTallyPlasticBase,       // a type-6 sample took the delta coat / the diffuse base
                 kTallyEmitterAfterCoat,                      // an emitter or sky reached after a sampled type-6 coat: emitter density 0, weight 1
                 kTallyRoughPlasticCoat, kTallyRoughPlasticBase,      // a type-7 sample took the GGX coat (and lived) / the base
                 kTallyRoughPlasticFailed,                    // a type-7 coat sample with pm == 0 or wo.z <= 0: a direction with value 0
                 kTallyPlasticFromBehind,                     // cos_i <= 0 at a one-sided entry of either type: the sample fails
                 kTallyPlasticBackFace,                       // a twosided entry of either type met from the back
                 kTallyNullOverPlastic,                       // a mask's null lobe at an entry whose nested BSDF is a plastic of either type
                 kTallyRRAfterCoat,                           // Russian roulette ended the path after a coat sample of either type
                 // the spot's falloff, the three delta lights told apart and the lens (D23, D24), appended; kTallyPointOccluded / Unoccluded
                 // keep counting every delta light
                 kTallySpotBeam, kTallySpotRamp,              // a spot's next-event sample with c >= cos_beam / strictly inside the ramp with f != 0
                 kTallySpotDark,                              // ... with f == 0: pdf 0, no shadow ray
                 kTallySpotOccluded, kTallySpotUnoccluded, kTallySunOccluded, kTallySunUnoccluded,
                 kTallyLensDiskFirst, kTallyLensDiskSecond,   // the concentric map's x x > y y branch / the other one, per camera ray of a render
                 kTallyCount };
static const int kTallyCountPlastics = (int) kTallySpotBeam;     // what msk_oracle_path_tally_count_all answered when it was introduced
static std::atomic<uint64_t> g_path[kTallyCount];
struct PathTallies { uint64_t v[kTallyCount] = {}; };
static thread_local PathTallies tl_path;
static inline void tally(PathTally t) { tl_path.v[t] += 1; }
static void path_flush() { for (int i = 0; i < kTallyCount; ++i) { g_path[i].fetch_add(tl_path.v[i], std::memory_order_relaxed); tl_path.v[i] = 0; } }
// Named events of the `direct` integrator (msk_oracle_direct_tallies; the path tallies' mechanism): which branches of direct_sample a
// render reached
enum DirectTally { kDirPrimaryMissEnv, kDirPrimaryEmitterSeen, kDirPrimaryEmitterHidden, kDirTwosidedFlipped, kDirLightSkippedDelta,
                   kDirLightAreaVisible, kDirLightAreaOccluded, kDirLightAreaBack,      // Back: pdf = 0, the sampled point faces away
                   kDirLightConstantSky, kDirLightImage, kDirLightPointVisible, kDirLightPointOccluded,
                   kDirLightLastEmitter,      // the selection took the last emitter of several
                   kDirBsdfNotTraced,         // the sample failed or its value is zero at every wavelength
                   kDirBsdfEmitterFrontMis,   // an area emitter's front with 0 < w_b < 1
                   kDirBsdfEmitterBack, kDirBsdfNonEmitter, kDirBsdfMissImage, kDirBsdfMissConstant, kDirBsdfMissNothing,
                   kDirBsdfEmitterAfterDelta, // an emitter or environment after a delta lobe: p_e = 0, weight exactly 1
                   // appended: the light loop tells spot from sun from point (kDirLightPointVisible / Occluded keep counting every delta light)
                   kDirLightSpotVisible, kDirLightSpotOccluded, kDirLightSpotDark,      // Dark: f == 0, the sample is skipped
                   kDirLightSunVisible, kDirLightSunOccluded, kDirLightPointOnlyVisible, kDirLightPointOnlyOccluded,
                   kDirTallyCount };
static const int kDirTallyCountFirst = (int) kDirLightSpotVisible;      // the twenty-one msk_oracle_direct_tally_count keeps answering for
static std::atomic<uint64_t> g_direct[kDirTallyCount];
struct DirectTallies { uint64_t v[kDirTallyCount] = {}; };
static thread_local DirectTallies tl_direct;
static inline void tally(DirectTally t) { tl_direct.v[t] += 1; }
static void direct_flush() { for (int i = 0; i < kDirTallyCount; ++i) { g_direct[i].fetch_add(tl_direct.v[i], std::memory_order_relaxed); tl_direct.v[i] = 0; } }
// what a render worker or a ray batch calls when it ends: this thread's intersection, path AND direct tallies into the totals
static void tallies_flush() { isect_flush(); path_flush(); direct_flush(); }

static inline float xor_sign(float a, uint32_t sgn) {
    uint32_t b; std::memcpy(&b, &a, 4); b ^= sgn; std::memcpy(&a, &b, 4); return a;
}
// Embree 3 MoellerTrumboreIntersector1 (see header).  tfar is the ray's
// ORIGINAL maxt: the closest hit is chosen afterwards by (t, prim) so that the
// result does not depend on the order triangles are visited in.
// D10: the hit point must also lie in the triangle's own bounding box grown by `pad`.  Moeller-Trumbore alone accepts
// points up to a few tenths of a unit outside sliver triangles (ill-conditioned barycentrics), and for a ray that is
// numerically parallel to the triangle's plane the arithmetic above can accept "hits" far outside the triangle
// (|den| ~ 1e-7 |Ng|: t = T/|den| is noise); whether such a hit is ever reported then depends on whether the ray happens
// to enter a BVH node containing the triangle — in Embree as much as here.  The predicate makes the answer a property of
// the ray and the triangle alone, so brute force and every conservative tree agree.
static inline bool intersect_triangle(const Tri &tr, const Ray &ray, float *t, float *u, float *v, float pad) {
    const V3 e1 = tr.p0 - tr.p1;           // TriangleM: e1 = v0 - v1
    const V3 e2 = tr.p2 - tr.p0;           //            e2 = v2 - v0
    const V3 ng = cross(e2, e1);           // tri_Ng = cross(e2, e1)
    const V3 C = tr.p0 - ray.o;
    const V3 R = cross(C, ray.d);
    const float den = dot(ng, ray.d);
    const float abs_den = std::fabs(den);
    uint32_t sgn; std::memcpy(&sgn, &den, 4); sgn &= 0x80000000u;
    const float U = xor_sign(dot(R, e2), sgn);
    const float V = xor_sign(dot(R, e1), sgn);
    if (!(den != 0.f && U >= 0.f && V >= 0.f && U + V <= abs_den)) return false;
    const float T = xor_sign(dot(ng, C), sgn);
    if (!(abs_den * ray.mint < T && T <= abs_den * ray.maxt)) return false;
    const float rcp = 1.f / abs_den;
    *t = T * rcp;
    *u = std::min(U * rcp, 1.f);
    *v = std::min(V * rcp, 1.f);
    // D10 bounds predicate: the reported hit point o + t d must lie in the bounding box of the triangle as the intersector
    // holds it (v0, v0 - e1, v0 + e2), grown by `pad`
    const V3 q1 = tr.p0 - e1, q2 = tr.p0 + e2;
    const float px = ray.o.x + *t * ray.d.x, py = ray.o.y + *t * ray.d.y, pz = ray.o.z + *t * ray.d.z;
    const bool inside =
           px >= std::min(tr.p0.x, std::min(q1.x, q2.x)) - pad && px <= std::max(tr.p0.x, std::max(q1.x, q2.x)) + pad &&
           py >= std::min(tr.p0.y, std::min(q1.y, q2.y)) - pad && py <= std::max(tr.p0.y, std::max(q1.y, q2.y)) + pad &&
           pz >= std::min(tr.p0.z, std::min(q1.z, q2.z)) - pad && pz <= std::max(tr.p0.z, std::max(q1.z, q2.z)) + pad;
    tl_isect.v[2] += 1;
    if (!inside) { tl_isect.v[3] += 1; tl_isect.rej = true; tl_isect.rej_t = std::min(tl_isect.rej_t, *t); }
    return inside;
}

static inline bool box_hit(const BVHNode &n, const Ray &r, V3 inv, float tbest) {
    float tmin = r.mint, tmax = tbest;
    float a, b;
    a = (n.lo.x - r.o.x) * inv.x; b = (n.hi.x - r.o.x) * inv.x;
    tmin = std::fmax(tmin, std::fmin(a, b)); tmax = std::fmin(tmax, std::fmax(a, b));
    a = (n.lo.y - r.o.y) * inv.y; b = (n.hi.y - r.o.y) * inv.y;
    tmin = std::fmax(tmin, std::fmin(a, b)); tmax = std::fmin(tmax, std::fmax(a, b));
    a = (n.lo.z - r.o.z) * inv.z; b = (n.hi.z - r.o.z) * inv.z;
    tmin = std::fmax(tmin, std::fmin(a, b)); tmax = std::fmin(tmax, std::fmax(a, b));
    return tmin <= tmax * 1.0000004f;
}

static Hit closest_hit(const Scene &sc, const Ray &ray) {
    Hit best{kInf, 0, 0, 0xffffffffu, false};
    bool tied = false;
    tl_isect.v[0] += 1; tl_isect.rej = false; tl_isect.rej_t = kInf;
    auto consider = [&](uint32_t prim) {
        float t, u, v;
        if (intersect_triangle(sc.tris[prim], ray, &t, &u, &v, sc.tri_pad)) {
            if (best.valid && t == best.t) { tl_isect.v[7] += 1; tied = true; }
            else if (!best.valid || t < best.t) tied = false;
            if (!best.valid || t < best.t || (t == best.t && prim < best.prim))
                best = Hit{t, u, v, prim, true};
        }
    };
    if (!sc.use_bvh || sc.nodes.empty()) {
        for (uint32_t p = 0; p < sc.tris.size(); ++p) consider(p);
    } else {
        V3 inv = mk3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
        int stack[64]; int sp = 0; stack[sp++] = 0;
        while (sp) {
            const BVHNode &n = sc.nodes[stack[--sp]];
            if (!box_hit(n, ray, inv, best.valid ? best.t : ray.maxt)) continue;
            if (n.left < 0) { for (int i = 0; i < n.count; ++i) consider(sc.tri_order[n.first + i]); }
            else { stack[sp++] = n.left; stack[sp++] = n.right; }
        }
    }
    // scene.cpp:234  `if (rh.ray.tfar != ray.maxt)`
    if (best.valid && best.t == ray.maxt) best.valid = false;
    if (tl_isect.rej && (!best.valid || tl_isect.rej_t < best.t)) tl_isect.v[4] += 1;
    if (best.valid && tied) tl_isect.v[6] += 1;
    return best;
}

static bool any_hit_walk(const Scene &sc, const Ray &ray);
static bool any_hit(const Scene &sc, const Ray &ray) {   // scene.cpp:255-273
    tl_isect.v[1] += 1; tl_isect.rej = false;
    const bool occluded = any_hit_walk(sc, ray);
    if (!occluded && tl_isect.rej) tl_isect.v[5] += 1;
    return occluded;
}
static bool any_hit_walk(const Scene &sc, const Ray &ray) {
    float t, u, v;
    if (!sc.use_bvh || sc.nodes.empty()) {
        for (uint32_t p = 0; p < sc.tris.size(); ++p)
            if (intersect_triangle(sc.tris[p], ray, &t, &u, &v, sc.tri_pad)) return true;
        return false;
    }
    V3 inv = mk3(1.f / ray.d.x, 1.f / ray.d.y, 1.f / ray.d.z);
    int stack[64]; int sp = 0; stack[sp++] = 0;
    while (sp) {
        const BVHNode &n = sc.nodes[stack[--sp]];
        if (!box_hit(n, ray, inv, ray.maxt)) continue;
        if (n.left < 0) {
            for (int i = 0; i < n.count; ++i)
                if (intersect_triangle(sc.tris[sc.tri_order[n.first + i]], ray, &t, &u, &v, sc.tri_pad)) return true;
        } else { stack[sp++] = n.left; stack[sp++] = n.right; }
    }
    return false;
}

// ===========================================================================
// a8  hit -> SceneInteraction  (mesh.cpp:50-101, interaction.cpp:23-37,
//     interaction.h:55-60)
// ===========================================================================
struct Interaction {
    float t = kInf;
    V3 p, n, wi;
    V2 uv;
    Frame sh;
    uint32_t prim = 0, mesh = 0;
    bool valid() const { return t != kInf; }
};

static Interaction compute_interaction(const Scene &sc, const Ray &ray, const Hit &h) {
    Interaction si;
    if (!h.valid) { si.t = kInf; si.wi = -ray.d; return si; }      // scene.cpp:247-251
    uint32_t mesh = sc.tri_mesh[h.prim];
    const msk_mesh_desc &md = sc.meshes[mesh];
    const uint32_t *fi = sc.face(mesh, h.prim - md.first_face);
    float b1 = h.u, b2 = h.v, b0 = 1.f - b1 - b2;                  // mesh.cpp:53
    V3 p0 = sc.vertex_position(mesh, fi[0]), p1 = sc.vertex_position(mesh, fi[1]),
       p2 = sc.vertex_position(mesh, fi[2]);
    V3 dp0 = p1 - p0, dp1 = p2 - p0;
    si.t = h.t;
    si.p = p0 * b0 + p1 * b1 + p2 * b2;                            // mesh.cpp:64
    si.n = normalized(cross(dp0, dp1));                            // mesh.cpp:65
    si.uv = V2{h.u, h.v};
    V3 dp_du, dp_dv;
    coordinate_system(si.n, &dp_du, &dp_dv);                       // mesh.cpp:67
    if (md.has_texcoords) {                                        // mesh.cpp:68-80
        V2 uv0 = sc.vertex_texcoord(mesh, fi[0]), uv1 = sc.vertex_texcoord(mesh, fi[1]),
           uv2 = sc.vertex_texcoord(mesh, fi[2]);
        si.uv = V2{uv0.x * b0 + uv1.x * b1 + uv2.x * b2, uv0.y * b0 + uv1.y * b1 + uv2.y * b2};
        V2 duv0{uv1.x - uv0.x, uv1.y - uv0.y}, duv1{uv2.x - uv0.x, uv2.y - uv0.y};
        float det = duv0.x * duv1.y - duv0.y * duv1.x, inv_det = 1.f / det;
        if (det != 0.f) {
            dp_du = (dp0 * duv1.y - dp1 * duv0.y) * inv_det;
            dp_dv = (dp0 * (-duv1.x) + dp1 * duv0.x) * inv_det;
        }
    }
    if (md.has_normals) {                                          // mesh.cpp:81-96
        V3 n0 = sc.vertex_normal(mesh, fi[0]), n1 = sc.vertex_normal(mesh, fi[1]),
           n2 = sc.vertex_normal(mesh, fi[2]);
        si.sh.n = normalized(n0 * b0 + n1 * b1 + n2 * b2);
    } else {
        si.sh.n = si.n;
    }
    si.prim = h.prim; si.mesh = mesh;
    // interaction.h:55-60 initialize_sh_frame
    V3 ff = (-si.sh.n) * dot(si.sh.n, dp_du) + dp_du;
    si.sh.s = normalized(ff);
    si.sh.t = cross(si.sh.n, si.sh.s);
    si.wi = si.sh.to_local(-ray.d);                                // interaction.cpp:31
    return si;
}

// ===========================================================================
// a12  spectra
// ===========================================================================
// spectra/regular.cpp:73-91 eval_pdf on the table's own grid (D65: [360,830], 95 samples, interval 5).
// The segment index: `x.cast<uint32_t>().cwiseMin(size - 2).cwiseMax(0)` in the reference.  Above the table that is size - 2 (the
// last segment continued linearly).  BELOW it the reference converts a negative float to uint32_t — undefined in C++; the
// restatement takes index 0 there (the first segment continued linearly: what the cwiseMax(0) is written for, and what the
// device's saturating conversion gives).  Wavelengths are sampled in [360, 830]: D65 and CIE never see either case.
static S4 regular_eval(const Scene::RegularTable &t, S4 wl) {
    const uint32_t last = (uint32_t) t.pdf.size() - 2u;
    S4 r;
    for (int i = 0; i < 4; ++i) {
        float x = (wl.v[i] - t.range_x) * t.inv_interval;
        uint32_t idx = x > 0.f ? std::min((uint32_t) std::min(x, 4.0e9f), last) : 0u;
        float y0 = t.pdf[idx], y1 = t.pdf[idx + 1];
        float w1 = x - (float) idx, w0 = 1.f - w1;
        r.v[i] = w0 * y0 + w1 * y1;
    }
    return r;
}
// spectra/srgb_d65.cpp:34-36; a `regular` radiance (AreaLight::m_radiance->eval, area.cpp:51-54): the table as it stands
static S4 emitter_radiance(const Scene &sc, int e, S4 wl) {
    if (sc.emitters[e].radiance_regular) return regular_eval(sc.emitter_table[e], wl);
    return regular_eval(sc.emitter_table[e], wl) * srgb_model_eval(sc.emitters[e].radiance, wl);
}
// core/spectrum.h:82-115 cie1931_xyz + spectrum_to_xyz
static void spectrum_to_xyz(const Scene &sc, S4 value, S4 wl, float xyz[3]) {
    S4 X, Y, Z;
    for (int s = 0; s < 4; ++s) {
        float t = (wl.v[s] - 360.f) * ((MSK_CIE_SAMPLES - 1) / (830.f - 360.f));
        uint32_t i0 = std::min(std::max((uint32_t) t, 0u), (uint32_t) (MSK_CIE_SAMPLES - 2)), i1 = i0 + 1;
        float w1 = t - (float) i0, w0 = 1.f - w1;
        X.v[s] = w0 * sc.cie[i0] + w1 * sc.cie[i1];
        Y.v[s] = w0 * sc.cie[MSK_CIE_SAMPLES + i0] + w1 * sc.cie[MSK_CIE_SAMPLES + i1];
        Z.v[s] = w0 * sc.cie[2 * MSK_CIE_SAMPLES + i0] + w1 * sc.cie[2 * MSK_CIE_SAMPLES + i1];
    }
    xyz[0] = mean4(X * value); xyz[1] = mean4(Y * value); xyz[2] = mean4(Z * value);
}

// ===========================================================================
// samplers (a16 + D2)
// ===========================================================================
struct Sampler {
    int mode;
    PCG32 rng;          // MSK_RNG_PCG_BLOCK: the block's stream (independent.cpp:28-35)
    uint64_t key = 0;   // MSK_RNG_COUNTER
    // dimension pairs: 0 = film position, 1 = (wavelength, -), 2 = aperture,
    // 3+3(k-1)+{0: NEE, 1: (bsdf sample1, rr), 2: bsdf direction}, k = depth
    std::vector<uint32_t> *log = nullptr;   // (msk_oracle_direct_terms) every pair index drawn from, in order
    void pair(uint32_t idx, float *a, float *b) {
        if (log) log->push_back(idx);
        if (mode == MSK_RNG_COUNTER) counter_pair(key, idx, a, b);
        else { *a = rng.next_float32(); *b = rng.next_float32(); }
    }
    float single(uint32_t idx, int lo) {
        if (log) log->push_back(idx);
        if (mode == MSK_RNG_COUNTER) { float a, b; counter_pair(key, idx, &a, &b); return lo ? b : a; }
        return rng.next_float32();
    }
};

// ===========================================================================
// a3  PerspectiveCamera::sample_ray (sensors/perspective.cpp:22-42)
// ===========================================================================
static V3 apply_point(const float m[16], V3 p) {   // transform.h:127-135, row-major m
    // Eigen 4x4 * vec4 (coeff-wise lazy product, left to right), then / w
    float r[4];
    for (int i = 0; i < 4; ++i)
        r[i] = ((m[i * 4 + 0] * p.x + m[i * 4 + 1] * p.y) + m[i * 4 + 2] * p.z) + m[i * 4 + 3] * 1.f;
    return mk3(r[0] / r[3], r[1] / r[3], r[2] / r[3]);
}
static V3 apply_vector(const float m[16], V3 v) {  // transform.h:123-125, 3x3 block, R2
    return mk3(m[0] * v.x + (m[1] * v.y + m[2] * v.z), m[4] * v.x + (m[5] * v.y + m[6] * v.z),
               m[8] * v.x + (m[9] * v.y + m[10] * v.z));
}
// msk_gpu.h at msk_lens_desc (D24), steps 1 to 6, each fp32 operation on its own.  `counted`: a render's ray (the disk map's branch is tallied)
static Ray lens_ray(const Scene &sc, V2 pos, V2 aperture, bool counted) {
    const V3 near_p = apply_point(sc.camera.sample_to_camera, mk3(pos.x, pos.y, 0.f));                 // 1
    int branch = 0;
    const V2 disk = square_to_uniform_disk_concentric(aperture, &branch);                                // 2
    if (counted && branch) tally(branch == 1 ? kTallyLensDiskFirst : kTallyLensDiskSecond);              // (the branch the map itself reports)
    const float lx = disk.x * sc.lens_radius, ly = disk.y * sc.lens_radius;
    const float ft = sc.lens_focus / near_p.z;                                                            // 3
    const V3 fp = mk3(near_p.x * ft, near_p.y * ft, near_p.z * ft);
    const V3 dl = normalized(mk3(fp.x - lx, fp.y - ly, fp.z));                                            // 4
    const float inv_z = 1.f / dl.z;
    Ray ray;
    ray.mint = sc.camera.near_clip * inv_z;
    ray.maxt = sc.camera.far_clip * inv_z;
    ray.o = apply_point(sc.camera.to_world, mk3(lx, ly, 0.f));                                            // 5
    ray.d = apply_vector(sc.camera.to_world, dl);                                                         // 6
    return ray;
}
// aperture: read by a scene with a lens only
static Ray camera_ray(const Scene &sc, float wavelength_sample, V2 pos, S4 *wl, S4 *weight, V2 aperture = V2{0.5f, 0.5f}, bool counted = false) {
    sample_wavelength(wavelength_sample, wl, weight);              // perspective.cpp:26-28
    if (sc.has_lens) return lens_ray(sc, pos, aperture, counted);
    V3 near_p = apply_point(sc.camera.sample_to_camera, mk3(pos.x, pos.y, 0.f));
    V3 d = normalized(near_p);
    float inv_z = 1.f / d.z;
    Ray ray;
    ray.mint = sc.camera.near_clip * inv_z;
    ray.maxt = sc.camera.far_clip * inv_z;
    ray.o = apply_point(sc.camera.to_world, mk3(0.f, 0.f, 0.f));
    ray.d = apply_vector(sc.camera.to_world, d);
    return ray;
}

// ===========================================================================
// a9/a10  emitter sampling
// ===========================================================================
// ---------------------------------------------------------------------------
// the `envmap` emitter (msk_gpu.h at msk_envmap_desc; D11-D13), fp32, one operation at a time
// ---------------------------------------------------------------------------
static const float kEnvEps2 = 3.5527136788005009e-15f;              // eps^2, eps = 2^-24
static const float kOneBelow = 1.f - 5.9604644775390625e-08f;       // 1 - 2^-24
// direction -> (u, v) and sin theta: dl = R^T d
static V2 env_dir_to_uv(const Scene::Envmap &m, V3 d, float *sin_theta) {
    const float *r = m.R;
    const float lx = r[0] * d.x + (r[3] * d.y + r[6] * d.z), ly = r[1] * d.x + (r[4] * d.y + r[7] * d.z), lz = r[2] * d.x + (r[5] * d.y + r[8] * d.z);
    const float s2 = lx * lx + lz * lz;
    float u = det_atan2(lx, -lz) / kTwoPi;
    u = u - std::floor(u);
    if (!(u < 1.f)) u = 0.f;
    const float v = det_atan2(std::sqrt(s2), ly) / kPi;
    *sin_theta = std::sqrt(s2 < kEnvEps2 ? kEnvEps2 : s2);
    return V2{u, v};
}
static S4 env_texel(const Scene::Envmap &m, int j, int i, S4 wl) {
    const float *t = &m.texels[((size_t) j * m.W + (size_t) i) * 4];
    return srgb_model_eval(t, wl) * t[3];
}
// L(u, v, l) = T_e(l) * bilerp(w_k S(coeff_k, l)): u wraps, v clamps at the poles
static S4 env_radiance(const Scene &sc, V2 uv, S4 wl) {
    const Scene::Envmap &m = sc.envmap;
    const int W = (int) m.W, H = (int) m.H;
    const float px = uv.x * (float) W - 0.5f;
    const float fi = std::floor(px), tx = px - fi;
    int i0 = (int) fi;
    if (i0 < 0) i0 = W - 1;
    if (i0 >= W) i0 = 0;
    const int i1 = i0 + 1 >= W ? 0 : i0 + 1;
    const float py = uv.y * (float) H - 0.5f;
    const float fj = std::floor(py), ty = py - fj;
    const int j = (int) fj;
    const int j0 = std::min(std::max(j, 0), H - 1), j1 = std::min(std::max(j + 1, 0), H - 1);
    if (j < 0 || j + 1 > H - 1) tally(kTallyPoleClamp);
    const S4 s00 = env_texel(m, j0, i0, wl), s10 = env_texel(m, j0, i1, wl), s01 = env_texel(m, j1, i0, wl), s11 = env_texel(m, j1, i1, wl);
    const S4 a = s00 + (s10 - s00) * tx, b = s01 + (s11 - s01) * tx;
    const S4 r = a + (b - a) * ty;
    return regular_eval(sc.emitter_table[sc.env], wl) * r;
}
static float env_pdf_cell(const Scene::Envmap &m, int i, int j, float sin_theta) {
    const float pr = m.marg[j + 1] - m.marg[j], pc = m.cond[j][i + 1] - m.cond[j][i];
    const float p = ((pr * pc) * (float) m.W) * (float) m.H;
    return p / (kTwoPiSqr * sin_theta);
}
// pdf(direction) from the uv of env_dir_to_uv: i = min((int) (u W), W - 1), j likewise
static float env_pdf(const Scene::Envmap &m, V2 uv, float sin_theta) {
    const int i = std::min((int) (uv.x * (float) m.W), (int) m.W - 1), j = std::min((int) (uv.y * (float) m.H), (int) m.H - 1);
    return env_pdf_cell(m, i, j, sin_theta);
}
// core/distribution.h:106-116 on a table of n + 1 entries: upper bound, clamp, the reused fraction kept below 1
static int env_search(const std::vector<float> &cdf, int n, float u, float *frac) {
    const int k = std::min(std::max((int) (std::upper_bound(cdf.begin(), cdf.begin() + n + 1, u) - cdf.begin()) - 1, 0), n - 1);
    const float f = (u - cdf[k]) / (cdf[k + 1] - cdf[k]);
    *frac = kOneBelow < f ? kOneBelow : f;
    return k;
}
static V3 env_sample(const Scene::Envmap &m, V2 u2, V2 *uv, float *pdf) {
    float dv, du;
    const int j = env_search(m.marg, (int) m.H, u2.y, &dv);
    const int i = env_search(m.cond[j], (int) m.W, u2.x, &du);
    const float u = ((float) i + du) / (float) m.W, v = ((float) j + dv) / (float) m.H;
    float st, ct, sp, cp;
    det_sincos(kPi * v, &st, &ct);
    det_sincos(kTwoPi * u, &sp, &cp);
    const float lx = sp * st, ly = ct, lz = -(cp * st);
    const float s2 = lx * lx + lz * lz;
    const float sin_theta = std::sqrt(s2 < kEnvEps2 ? kEnvEps2 : s2);
    const float *r = m.R;
    *uv = V2{u, v};
    *pdf = env_pdf_cell(m, i, j, sin_theta);
    return mk3(r[0] * lx + (r[1] * ly + r[2] * lz), r[3] * lx + (r[4] * ly + r[5] * lz), r[6] * lx + (r[7] * ly + r[8] * lz));
}

struct DirectSample { V3 p, n, d; float dist, pdf; int emitter; bool point = false; int falloff = 0; };      // falloff (tallies only): a spot's branch, 1 beam, 2 ramp, 3 dark

// core/distribution.h:106-116 Distribution1D::sample / sample_reuse
static uint32_t distr_sample(const std::vector<float> &cdf, float u) {
    auto it = std::upper_bound(cdf.begin(), cdf.end(), u);
    return (uint32_t) std::min(std::max((int) std::distance(cdf.begin(), it) - 1, 0), (int) cdf.size() - 2);
}
// msk_gpu.h at msk_point_desc: d = position - p; dist = sqrt(d.x d.x + (d.y d.y + d.z d.z)); inv = 1 / dist; d = d * inv; pdf = 1;
// value(l) = (I(l) * inv) * inv.  dist == 0 gives pdf = 0 and no contribution.
static S4 point_sample(V3 position, V3 p, S4 intensity, V3 *d_out, float *dist_out, float *pdf) {
    const V3 d = position - p;
    const float dist = std::sqrt(d.x * d.x + (d.y * d.y + d.z * d.z));
    *dist_out = dist;
    if (dist == 0.f) { *d_out = mk3(0.f, 0.f, 0.f); *pdf = 0.f; return s4(0.f); }
    const float inv = 1.f / dist;
    *d_out = d * inv;
    *pdf = 1.f;
    return (intensity * inv) * inv;
}
// mesh.cpp:103-133 sample_position + shape.cpp:64-78 sample_direct + area.cpp:32-45
static DirectSample emitter_sample_direct(const Scene &sc, int e, const Interaction &ref, V2 sample,
                                          S4 wl, S4 *spec) {
    const msk_emitter_desc &em = sc.emitters[e];
    if (em.type == MSK_EMITTER_POINT) {
        DirectSample ds;
        *spec = point_sample(sc.point_pos[e], ref.p, emitter_radiance(sc, e, wl), &ds.d, &ds.dist, &ds.pdf);
        ds.p = sc.point_pos[e]; ds.n = -ds.d; ds.emitter = e; ds.point = true;
        return ds;
    }
    if (em.type == MSK_EMITTER_SPOT) {
        // msk_gpu.h at msk_light_desc: the point light's d, dist, inv; c = -(d . a); the falloff tested in this order: c >= cos_beam gives
        // 1, c <= cos_cutoff gives 0, otherwise t = (c - cos_cutoff) / (cos_beam - cos_cutoff), f = (t * t) * (3 - 2 * t); f == 0: pdf = 0
        const Scene::Light &l = sc.lights[e];
        DirectSample ds;
        *spec = point_sample(l.position, ref.p, emitter_radiance(sc, e, wl), &ds.d, &ds.dist, &ds.pdf);
        ds.p = l.position; ds.n = -ds.d; ds.emitter = e; ds.point = true;
        if (ds.pdf != 0.f) {
            const float c = -(ds.d.x * l.direction.x + (ds.d.y * l.direction.y + ds.d.z * l.direction.z));
            float f;
            if (c >= l.cos_beam) { f = 1.f; ds.falloff = 1; }
            else if (c <= l.cos_cutoff) f = 0.f;
            else { const float t = (c - l.cos_cutoff) / (l.cos_beam - l.cos_cutoff); f = (t * t) * (3.f - 2.f * t); ds.falloff = 2; }
            *spec = *spec * f;
            if (f == 0.f) { ds.pdf = 0.f; *spec = s4(0.f); ds.falloff = 3; }
        }
        return ds;
    }
    if (em.type == MSK_EMITTER_DIRECTIONAL) {
        // msk_gpu.h at msk_light_desc: d = -w, dist = 2 * env_radius, pdf = 1, value(l) = E(l)
        const Scene::Light &l = sc.lights[e];
        DirectSample ds;
        ds.d = mk3(-l.direction.x, -l.direction.y, -l.direction.z);
        ds.dist = 2.f * sc.env_radius;
        ds.p = ref.p + ds.d * ds.dist; ds.n = -ds.d; ds.pdf = 1.f; ds.emitter = e; ds.point = true;
        *spec = emitter_radiance(sc, e, wl);
        return ds;
    }
    if (em.type == MSK_EMITTER_ENVMAP) {
        // msk_gpu.h at msk_envmap_desc: next-event value = L(uv) / pdf_omega, dist = 2 * env_radius; pdf 0 gives no contribution
        DirectSample ds;
        V2 uv;
        ds.d = env_sample(sc.envmap, sample, &uv, &ds.pdf);
        ds.dist = 2.f * sc.env_radius;
        ds.p = ref.p + ds.d * ds.dist;
        ds.n = -ds.d;
        ds.emitter = e;
        *spec = ds.pdf != 0.f ? env_radiance(sc, uv, wl) / ds.pdf : s4(0.f);
        return ds;
    }
    if (em.type == MSK_EMITTER_CONSTANT) {
        // constant.cpp:53-72.  D8: the reference evaluates the radiance on a default-constructed interaction
        // (uninitialised wavelengths); the wavelengths of the reference point are used, as area.cpp:35-36 does.
        DirectSample ds;
        ds.d = square_to_uniform_sphere(sample);
        ds.dist = 2.f * sc.env_radius;
        ds.p = ref.p + ds.d * ds.dist;
        ds.n = -ds.d;
        ds.pdf = kInvFourPi;
        ds.emitter = e;
        *spec = emitter_radiance(sc, e, wl) / ds.pdf;
        return ds;
    }
    uint32_t mesh = (uint32_t) em.mesh_id;
    const std::vector<float> &cdf = sc.mesh_cdf[mesh];
    uint32_t face_idx = distr_sample(cdf, sample.y);
    sample.y = (sample.y - cdf[face_idx]) / (cdf[face_idx + 1] - cdf[face_idx]);
    const uint32_t *fi = sc.face(mesh, face_idx);
    V3 p0 = sc.vertex_position(mesh, fi[0]), p1 = sc.vertex_position(mesh, fi[1]),
       p2 = sc.vertex_position(mesh, fi[2]);
    V3 e0 = p1 - p0, e1 = p2 - p0;
    V2 b = square_to_uniform_triangle(sample);
    DirectSample ds;
    ds.p = p0 + e0 * b.x + e1 * b.y;
    V3 ng = normalized(cross(e0, e1)), ns = ng;
    if (sc.meshes[mesh].has_normals) {
        V3 n0 = sc.vertex_normal(mesh, fi[0]), n1 = sc.vertex_normal(mesh, fi[1]),
           n2 = sc.vertex_normal(mesh, fi[2]);
        ns = normalized(n0 * (1.f - b.x - b.y) + n1 * b.x + n2 * b.y);
    }
    ds.n = ns;
    ds.pdf = 1.f / sc.mesh_area[mesh];
    // shape.cpp:66-75
    ds.d = ds.p - ref.p;
    float dist_squared = squared_norm(ds.d);
    ds.dist = std::sqrt(dist_squared);
    ds.d = ds.d / ds.dist;
    float dp = std::fabs(dot(ds.d, ds.n));
    ds.pdf *= (dp != 0.f) ? dist_squared / dp : 0.f;
    ds.emitter = e;
    // area.cpp:39-44
    if (dot(ds.d, ds.n) < 0.f && ds.pdf != 0.f) {
        *spec = emitter_radiance(sc, e, wl) / ds.pdf;
    } else {
        ds.pdf = 0;
        *spec = s4(0.f);
    }
    return ds;
}
// scene.cpp:68-103
static DirectSample sample_emitter_direct(const Scene &sc, const Interaction &ref, V2 sample, S4 wl,
                                          S4 *spec, uint64_t *shadow_rays, S4 *unoccluded = nullptr, bool *occluded_out = nullptr) {
    DirectSample ds; ds.pdf = 0; ds.emitter = -1;
    size_t n = sc.emitters.size();
    if (n == 0) { *spec = s4(0.f); return ds; }
    if (n == 1) {
        ds = emitter_sample_direct(sc, 0, ref, sample, wl, spec);
    } else {
        float light_sel_pdf = 1.f / n;
        uint32_t index = std::min(uint32_t(sample.x * (float) n), (uint32_t) n - 1);
        sample.x = (sample.x - index * light_sel_pdf) * n;
        ds = emitter_sample_direct(sc, (int) index, ref, sample, wl, spec);
        ds.pdf *= light_sel_pdf;
        *spec = *spec * (float) n;
    }
    if (ds.pdf != 0.f) {                                           // scene.cpp:90-97
        Ray ray{ref.p, ds.d, kRayEpsilon * (1.f + max_abs(ref.p)), ds.dist * (1.f - kShadowEpsilon)};
        ++*shadow_rays;
        const bool occluded = any_hit(sc, ray);
        if (g_trace_path)
            std::printf("  shadow ray o %.9g %.9g %.9g tmin %.9g d %.9g %.9g %.9g tmax %.9g occluded %d\n", ray.o.x, ray.o.y, ray.o.z, ray.mint,
                        ray.d.x, ray.d.y, ray.d.z, ray.maxt, (int) occluded);
        if (unoccluded) *unoccluded = *spec;             // (tallies only)
        if (occluded_out) *occluded_out = occluded;
        if (occluded) *spec = s4(0.f);
    }
    return ds;
}
// scene.cpp:105-112 + shape.cpp:80-86 + mesh.cpp:135-137
static float pdf_emitter_direct(const Scene &sc, const DirectSample &ds) {
    int e = sc.emitters.size() == 1 ? 0 : ds.emitter;
    float pdf;
    if (sc.emitters[e].type == MSK_EMITTER_CONSTANT) {
        pdf = kInvFourPi;                                          // constant.cpp:74-76
    } else {
        pdf = 1.f / sc.mesh_area[sc.emitters[e].mesh_id];
        float dp = std::fabs(dot(ds.d, ds.n));
        pdf *= (dp != 0.f) ? (ds.dist * ds.dist) / dp : 0.f;
    }
    return sc.emitters.size() == 1 ? pdf : pdf * (1.f / sc.emitters.size());
}
// area.cpp:51-54
static S4 emitter_eval(const Scene &sc, int e, const Interaction &si, S4 wl) {
    return si.wi.z > 0.f ? emitter_radiance(sc, e, wl) : s4(0.f);
}

// path.cpp:127-131
static float mis_weight(float pdf_a, float pdf_b) {
    pdf_a *= pdf_a; pdf_b *= pdf_b;
    return pdf_a > 0.f ? pdf_a / (pdf_a + pdf_b) : 0.f;
}

// ===========================================================================
// BSDFs: a11 diffuse (bsdfs/diffuse.cpp:18-57); §8(f)1 rough conductor
// (bsdfs/roughconductor.cpp:52-120, render/microfacet.h:11-44,145-175,
// render/fresnel.h:65-88) and the twosided adapter (bsdfs/twosided.cpp:38-101); the
// rough dielectric (bsdfs/roughdielectric.cpp:57-190) and the smooth one
// (bsdfs/dielectric.cpp:26-82, render/fresnel.h:12-14,22-27,37-63).
//
// The rough conductor has NO runnable reference (not compiled, written
// against Color3/eval_3, default distribution Beckmann is unimplemented).  This
// restates its arithmetic with the adaptation DESIGN.md §rough conductor states:
// GGX only; alpha is a float property; eta, k and specular_reflectance are
// spectra evaluated at the path's four wavelengths (value = scale * S(coeff, l)).
// ===========================================================================
struct BSDFSampleRec { V3 wo; float pdf, eta; uint32_t sampled_type; };   // render/bsdf.h:60-80
enum : uint32_t { kDiffuseReflection = 1u, kGlossyReflection = 2u, kGlossyTransmission = 4u, kDeltaReflection = 8u, kDeltaTransmission = 16u,
                  kDelta = kDeltaReflection | kDeltaTransmission,       // BSDFFlags::Delta: what path.cpp:104 asks of sampled_type
                  kNull = 32u };                                        // a mask's null lobe (BSDFFlags::Null)

static S4 spectrum_eval(const Scene &sc, const msk_spectrum_desc &sp, S4 wl) {
    if (sp.regular) return regular_eval(sc.regular[sp.regular - 1], wl);          // RegularSpectrum::eval (regular.cpp:148)
    return srgb_model_eval(sp.coeff, wl) * sp.scale;
}

// render/microfacet.h:11-18
static float eval_ggx(V3 m, float au, float av) {
    float cos_theta2 = m.z * m.z;
    float beckman_exp = ((m.x * m.x / (au * au)) + (m.y * m.y) / (av * av)) / cos_theta2;
    float root = (1.f + beckman_exp) * cos_theta2;
    return 1.f / (kPi * au * av * root * root);
}
// render/microfacet.h:20-40
static V3 sample_ggx(V2 sample, float au, float av, float *pdf_out) {
    float phi_m = det_atan(au / av * det_tan(kPi + 2 * kPi * sample.y)) + kPi * std::floor(2 * sample.y + 0.5f);
    float sin_phi_m, cos_phi_m;
    det_sincos(phi_m, &sin_phi_m, &cos_phi_m);
    float cs = cos_phi_m / au, sn = sin_phi_m / av;
    float alpha_sqr = 1.f / (cs * cs + sn * sn);
    float tan_theta_m_sqr = alpha_sqr * sample.x / (1.f - sample.x);
    float cos_theta_m = 1.f / std::sqrt(1.f + tan_theta_m_sqr);
    float tmp = 1 + tan_theta_m_sqr / alpha_sqr;
    float pdf = kInvPi / (au * av * cos_theta_m * cos_theta_m * cos_theta_m * tmp * tmp);
    if (pdf < 1e-20f) pdf = 0;
    float sin_theta_m = safe_sqrt(1 - cos_theta_m * cos_theta_m);
    *pdf_out = pdf;
    return mk3(sin_theta_m * cos_phi_m, sin_theta_m * sin_phi_m, cos_theta_m);
}
// MicrofacetDistribution::eval (microfacet.h:104-121), GGX
static float distr_eval(V3 m, float au, float av) {
    if (m.z <= 0) return 0.0f;
    float result = eval_ggx(m, au, av);
    return result * m.z > 1e-20f ? result : 0.f;
}
// MicrofacetDistribution::smith_g1 (microfacet.h:145-172), GGX
static float smith_g1(V3 v, V3 m, float au, float av) {
    float xy_alpha_2 = (au * v.x) * (au * v.x) + (av * v.y) * (av * v.y), tan_theta_alpha_2 = xy_alpha_2 / (v.z * v.z);
    if (xy_alpha_2 == 0.f) return 1.f;
    if (dot(v, m) * v.z <= 0.f) return 0.f;
    return 2.f / (1.f + std::sqrt(1.f + tan_theta_alpha_2));
}
// render/fresnel.h:65-88, one wavelength
static float fresnel_conductor(float cos_theta_i, float eta_r, float eta_i) {
    float cos_theta_i_2 = cos_theta_i * cos_theta_i, sin_theta_i_2 = 1.f - cos_theta_i_2, sin_theta_i_4 = sin_theta_i_2 * sin_theta_i_2;
    float temp_1 = eta_r * eta_r - eta_i * eta_i - sin_theta_i_2;
    float a_2_pb_2 = std::sqrt(temp_1 * temp_1 + 4.f * eta_i * eta_i * eta_r * eta_r);
    float a = std::sqrt(.5f * (a_2_pb_2 + temp_1));
    float term_1 = a_2_pb_2 + cos_theta_i_2, term_2 = 2.f * cos_theta_i * a;
    float r_s = (term_1 - term_2) / (term_1 + term_2);
    float term_3 = a_2_pb_2 * cos_theta_i_2 + sin_theta_i_4, term_4 = term_2 * sin_theta_i_2;
    float r_p = r_s * (term_3 - term_4) / (term_3 + term_4);
    return .5f * (r_s + r_p);
}
static S4 fresnel_conductor4(float c, S4 eta, S4 k) {
    S4 r; for (int i = 0; i < 4; ++i) r.v[i] = fresnel_conductor(c, eta.v[i], k.v[i]); return r;
}
static float clamp_alpha(float a) { return std::max(a, 1e-4f); }   // MicrofacetDistribution::configure
// render/fresnel.h:37-63 fresnel(): F, cos_theta_t, eta_it, eta_ti
static void fresnel_dielectric(float cos_theta_i, float eta, float *F, float *cos_theta_t, float *eta_it, float *eta_ti) {
    if (cos_theta_i >= 0.f) { *eta_it = eta; *eta_ti = 1.f / eta; } else { *eta_it = 1.f / eta; *eta_ti = eta; }
    float cos_theta_t_sqr = 1.f - *eta_ti * *eta_ti * (1.f - cos_theta_i * cos_theta_i);
    float cos_theta_i_abs = std::fabs(cos_theta_i);
    float cos_theta_t_abs = safe_sqrt(cos_theta_t_sqr);
    float a_s = (cos_theta_i_abs - *eta_it * cos_theta_t_abs) / (cos_theta_i_abs + *eta_it * cos_theta_t_abs);
    float a_p = (cos_theta_t_abs - *eta_it * cos_theta_i_abs) / (cos_theta_t_abs + *eta_it * cos_theta_i_abs);
    float r;
    if (eta == 1.f || cos_theta_i_abs == 0.f) r = eta == 1.f ? 0.f : 1.f;
    else r = 0.5f * (a_s * a_s + a_p * a_p);
    *cos_theta_t = cos_theta_t_abs * std::copysign(1.f, -cos_theta_i);
    *F = r;
}
// bsdfs/roughdielectric.cpp:118-190 eval + pdf (both lobes enabled, TransportMode::Radiance)
static void roughdielectric_eval_pdf(const Scene &sc, const msk_bsdf_desc &b, V3 wi, V3 wo, S4 wl, S4 *val, float *pdf) {
    *val = s4(0.f); *pdf = 0.f;
    const float cos_i = wi.z, cos_o = wo.z;
    if (cos_i == 0.f) return;
    const float au = clamp_alpha(b.alpha_u), av = clamp_alpha(b.alpha_v);
    const bool reflect = cos_i * cos_o > 0.f;
    const float eta = cos_i > 0.f ? b.ior_eta : b.ior_inv_eta, inv_eta = cos_i > 0.f ? b.ior_inv_eta : b.ior_eta;
    V3 m = normalized(wi + wo * (reflect ? 1.f : eta));
    m = m * std::copysign(1.f, m.z);
    float F, ct, e_it, e_ti;
    {   // eval
        float D = distr_eval(m, au, av);
        fresnel_dielectric(dot(wi, m), b.ior_eta, &F, &ct, &e_it, &e_ti);
        float G = smith_g1(wi, m, au, av) * smith_g1(wo, m, au, av);
        if (reflect) {
            *val = spectrum_eval(sc, b.specular_reflectance, wl) * (F * D * G) / (4.f * std::fabs(cos_i));
        } else {
            float scale = inv_eta * inv_eta;
            float denom = dot(wi, m) + eta * dot(wo, m);
            *val = spectrum_eval(sc, b.specular_transmittance, wl) *
                   std::fabs((scale * (1.f - F) * D * G * eta * eta * dot(wi, m) * dot(wo, m)) / (cos_i * (denom * denom)));
        }
    }
    // pdf
    if (dot(wi, m) * wi.z <= 0.f || dot(wo, m) * wo.z <= 0.f) return;
    float denom = dot(wi, m) + eta * dot(wo, m);
    float dwh_dwo = reflect ? 1.f / (4.f * dot(wo, m)) : (eta * eta * dot(wo, m)) / (denom * denom);
    float sau = au, sav = av;
    if (!b.sample_visible) { float sc = 1.2f - .2f * std::sqrt(std::fabs(wi.z)); sau *= sc; sav *= sc; }
    float prob = distr_eval(m, sau, sav) * m.z;
    prob *= reflect ? F : 1.f - F;
    *pdf = prob * std::fabs(dwh_dwo);
}
// bsdfs/roughdielectric.cpp:57-116 sample (both lobes enabled)
static S4 roughdielectric_sample(const Scene &sc, const msk_bsdf_desc &b, V3 wi, float sample1, V2 sample, S4 wl, BSDFSampleRec *bs) {
    const float cos_i = wi.z;
    const float au = clamp_alpha(b.alpha_u), av = clamp_alpha(b.alpha_v);
    float sau = au, sav = av;
    if (!b.sample_visible) { float sc = 1.2f - .2f * std::sqrt(std::fabs(cos_i)); sau *= sc; sav *= sc; }
    V3 m = sample_ggx(sample, sau, sav, &bs->pdf);
    if (bs->pdf == 0) return s4(0.f);
    float F, cos_t, eta_it, eta_ti;
    fresnel_dielectric(dot(wi, m), b.ior_eta, &F, &cos_t, &eta_it, &eta_ti);
    const bool selected_r = sample1 <= F;
    S4 weight = s4(1.f);
    bs->pdf *= selected_r ? F : (1.f - F);
    bs->eta = selected_r ? 1.f : eta_it;
    bs->sampled_type = selected_r ? kGlossyReflection : kGlossyTransmission;
    float dwh_dwo;
    if (selected_r) {
        bs->wo = m * 2.f * dot(wi, m) - wi;                               // fresnel.h:17-21
        weight = weight * spectrum_eval(sc, b.specular_reflectance, wl);
        dwh_dwo = 1.f / (4.f * dot(bs->wo, m));
    } else {
        bs->wo = m * (dot(wi, m) * eta_ti + cos_t) - wi * eta_ti;          // fresnel.h:30-35 refract(wi, m, cos_t, eta_ti)
        weight = weight * (eta_ti * eta_ti);
        float denom = dot(wi, m) + bs->eta * dot(bs->wo, m);
        dwh_dwo = (bs->eta * bs->eta) * dot(bs->wo, m) / (denom * denom);
    }
    if (b.sample_visible) weight = weight * smith_g1(bs->wo, m, au, av);
    else weight = weight * (smith_g1(wi, m, au, av) * smith_g1(bs->wo, m, au, av) * dot(wi, m) / (cos_i * m.z));
    bs->pdf *= std::fabs(dwh_dwo);
    return weight;
}
// bsdfs/dielectric.cpp:26-72 sample (both delta components enabled, TransportMode::Radiance).  The lobe is chosen by the x of the
// 2D sample (:37), sample1 is drawn by the caller and unused; reflect(wi) / refract(wi, cos_theta_t, eta_ti) are fresnel.h:12-14,22-27.
static S4 dielectric_sample(const Scene &sc, const msk_bsdf_desc &b, V3 wi, V2 sample, S4 wl, BSDFSampleRec *bs) {
    float r_i, cos_theta_t, eta_it, eta_ti;
    fresnel_dielectric(wi.z, b.ior_eta, &r_i, &cos_theta_t, &eta_it, &eta_ti);          // :31-32
    const float t_i = 1.f - r_i;
    const bool selected_r = sample.x <= r_i;                                             // :37
    bs->pdf = selected_r ? r_i : t_i;                                                    // :38
    bs->sampled_type = selected_r ? kDeltaReflection : kDeltaTransmission;               // :48-49
    bs->wo = selected_r ? mk3(-wi.x, -wi.y, wi.z) : mk3(-eta_ti * wi.x, -eta_ti * wi.y, cos_theta_t);   // :50-51
    bs->eta = selected_r ? 1.f : eta_it;                                                 // :52
    if (selected_r) return spectrum_eval(sc, b.specular_reflectance, wl);               // :55-56,61,65-66
    return spectrum_eval(sc, b.specular_transmittance, wl) * eta_ti * eta_ti;           // :57-58,61,67-70
}
// BSDFFlags::Smooth of bsdf->flags() (path.cpp:56): every BSDF here but `dielectric`, whose two components are delta (dielectric.cpp:21-23)
// and `conductor`, one delta reflection lobe (msk_gpu.h at MSK_BSDF_CONDUCTOR: "no next-event sample is taken at such a hit")
// (true for `plastic` too, D19: its diffuse lobe is smooth, the coat's delta mark belongs to the sample)
static bool bsdf_has_smooth_lobe(const msk_bsdf_desc &b) { return b.type != MSK_BSDF_DIELECTRIC && b.type != MSK_BSDF_CONDUCTOR; }
// msk_gpu.h at MSK_BSDF_CONDUCTOR: cos_i <= 0 fails (no direction); otherwise wo = (-wi.x, -wi.y, wi.z), pdf = 1, eta = 1,
// value(l) = specular_reflectance(l) * fresnel_conductor(cos_i, eta(l), k(l)), one product
static S4 conductor_sample(const Scene &sc, const msk_bsdf_desc &b, V3 wi, S4 wl, BSDFSampleRec *bs) {
    const float cos_i = wi.z;
    if (!(cos_i > 0.f)) return s4(0.f);
    bs->wo = mk3(-wi.x, -wi.y, wi.z);
    bs->pdf = 1.f;
    bs->eta = 1.f;
    bs->sampled_type = kDeltaReflection;
    return spectrum_eval(sc, b.specular_reflectance, wl) * fresnel_conductor4(cos_i, spectrum_eval(sc, b.eta, wl), spectrum_eval(sc, b.k, wl));
}

// msk_gpu.h at msk_texture_desc: uv' = to_uv (u, v, 1), each row a0 + (a1 + a2); f = x - floor(x) (repeat; can be exactly 1)
static V2 texture_frac_uv(const float *to_uv, V2 uv) {
    const float x = to_uv[0] * uv.x + (to_uv[1] * uv.y + to_uv[2] * 1.f);
    const float y = to_uv[3] * uv.x + (to_uv[4] * uv.y + to_uv[5] * 1.f);
    return V2{x - std::floor(x), y - std::floor(y)};
}
static int nearest_axis(float f, int n) { return std::min((int) (f * (float) n), n - 1); }
// bilinear: px = f n - 0.5; i0 = floor(px); t = px - i0; i0 < 0 -> n - 1; i0 >= n -> 0; i1 = i0 + 1, i1 >= n -> 0
static void bilinear_axis(float f, int n, int *i0, int *i1, float *t, bool *wrapped) {
    const float p = f * (float) n - 0.5f;
    const float fl = std::floor(p);
    *t = p - fl;
    int a = (int) fl;
    if (a < 0) { a = n - 1; *wrapped = true; }
    if (a >= n) { a = 0; *wrapped = true; }
    int b = a + 1;
    if (b >= n) { b = 0; *wrapped = true; }
    *i0 = a; *i1 = b;
}
// the lookup of MSK_TEXTURE_BITMAP / _NEAREST over any texel function: what a bitmap's reflectance and a mask's opacity share,
// "word for word"; value = a + ty (b - a) with a = s00 + tx (s10 - s00), b = s01 + tx (s11 - s01)
template <typename T, typename Texel> static T image_lookup(const float *to_uv, int W, int H, bool bilinear, V2 uv, Texel texel) {
    const V2 f = texture_frac_uv(to_uv, uv);
    if (!bilinear) return texel(nearest_axis(f.y, H), nearest_axis(f.x, W));
    int i0, i1, j0, j1; float tx, ty; bool wrapped = false;
    bilinear_axis(f.x, W, &i0, &i1, &tx, &wrapped);
    bilinear_axis(f.y, H, &j0, &j1, &ty, &wrapped);
    if (wrapped) tally(kTallyTexelWrap);
    const T s00 = texel(j0, i0), s10 = texel(j0, i1), s01 = texel(j1, i0), s11 = texel(j1, i1);
    const T a = s00 + (s10 - s00) * tx, b = s01 + (s11 - s01) * tx;
    return a + (b - a) * ty;
}
static S4 bitmap_eval(const Scene &sc, const msk_texture_desc &t, V2 uv, S4 wl) {
    const float *pool = sc.texels.data() + (size_t) t.first_texel * 3;
    return image_lookup<S4>(t.to_uv, (int) t.width, (int) t.height, t.type == MSK_TEXTURE_BITMAP, uv,
                            [&](int j, int i) { return srgb_model_eval(pool + ((size_t) j * t.width + (size_t) i) * 3, wl); });
}
// msk_gpu.h at msk_mask_desc: the opacity of entry `bsdf_id` at uv; 1 for an entry without a mask
static float mask_opacity(const Scene &sc, int bsdf_id, V2 uv) {
    if (sc.masks.empty() || sc.masks[bsdf_id].filter < 0) return 1.f;
    const Scene::Mask &m = sc.masks[bsdf_id];
    if (m.filter == 0) return m.opacity;
    return image_lookup<float>(m.to_uv, (int) m.W, (int) m.H, m.filter == 2, uv, [&](int j, int i) { return m.values[(size_t) j * m.W + (size_t) i]; });
}

// textures/checkerboard.cpp:24-33: which of the two colours the texture shows at uv.  The 3x3 product of
// Transform3f::transform_affine_point (core/transform.h:41-48) is Eigen's coefficient-based one: each row is
// a 3-element reduction a0 + (a1 + a2), like every other 3-vector sum here.
static const float *checkerboard_lookup(const msk_texture_desc &t, V2 uv) {
    const float x = t.to_uv[0] * uv.x + (t.to_uv[1] * uv.y + t.to_uv[2] * 1.f);
    const float y = t.to_uv[3] * uv.x + (t.to_uv[4] * uv.y + t.to_uv[5] * 1.f);
    const float u = x - std::floor(x), v = y - std::floor(y);
    return ((u > .5f) == (v > .5f)) ? t.color0 : t.color1;
}
// SmoothDiffuse::m_reflectance->eval(si) (diffuse.cpp:31,44): the coefficients of the spectrum the reflectance
// texture shows at the hit
struct Reflectance { const float *coeff; float scale; uint32_t regular; const msk_texture_desc *bitmap = nullptr; V2 uv = V2{0.f, 0.f}; };
static Reflectance reflectance_at(const Scene &sc, const msk_bsdf_desc &b, V2 uv) {
    if (b.reflectance_regular) return {b.reflectance, 1.f, b.reflectance_regular};
    if (b.reflectance_texture == 0) return {b.reflectance, b.reflectance_scale, 0u};
    const msk_texture_desc &t = sc.textures[b.reflectance_texture - 1];
    if (t.type == MSK_TEXTURE_BITMAP || t.type == MSK_TEXTURE_BITMAP_NEAREST) return {b.reflectance, 1.f, 0u, &t, uv};   // a spectrum, not coefficients
    return {checkerboard_lookup(t, uv), 1.f, 0u};
}
static S4 reflectance_eval(const Scene &sc, Reflectance r, S4 wl) {
    if (r.bitmap) return bitmap_eval(sc, *r.bitmap, r.uv, wl);
    if (r.regular) return regular_eval(sc.regular[r.regular - 1], wl);
    return srgb_model_eval(r.coeff, wl) * r.scale;
}

// ---------------------------------------------------------------------------
// `plastic` and `roughplastic` (msk_gpu.h at msk_bsdf_desc; D19-D21), fp32, one operation at a time, wi on the front side
// ---------------------------------------------------------------------------
static inline bool is_plastic(const msk_bsdf_desc &b) { return b.type == MSK_BSDF_PLASTIC || b.type == MSK_BSDF_ROUGHPLASTIC; }
// {fdr_int, ssw} of entry b of the scene; false for a descriptor that is not an entry of `sc` (the bare descriptors of the BSDF KAT hooks)
static bool plastic_k_of(const Scene &sc, const msk_bsdf_desc &b, Scene::PlasticK *k) {
    if (sc.bsdfs.empty() || &b < sc.bsdfs.data() || &b >= sc.bsdfs.data() + sc.bsdfs.size()) return false;
    const size_t i = (size_t) (&b - sc.bsdfs.data());
    if (i >= sc.plastic_k.size()) return false;
    *k = sc.plastic_k[i];
    return true;
}
static float fresnel_F(float cos_i, float eta) {
    float F, ct, e_it, e_ti;
    fresnel_dielectric(cos_i, eta, &F, &ct, &e_it, &e_ti);
    return F;
}
// F_i = fresnel_dielectric(cos_i, ior_eta), ps = F_i * ssw, pd = (1 - F_i) * (1 - ssw); cos_i <= 0 or ps + pd == 0 fails; otherwise
// ps = ps / (ps + pd), pd = 1 - ps
static bool plastic_lobes(const msk_bsdf_desc &b, float ssw, float cos_i, float *F_i, float *ps, float *pd) {
    if (!(cos_i > 0.f)) return false;
    *F_i = fresnel_F(cos_i, b.ior_eta);
    const float a = *F_i * ssw;
    const float d = (1.f - *F_i) * (1.f - ssw);
    const float s = a + d;
    if (s == 0.f) return false;
    *ps = a / s;
    *pd = 1.f - *ps;
    return true;
}
// D(l) * f with D(l) = rho(l) / (1 - fdr_int * rho(l)) when nonlinear, else rho(l) / (1 - fdr_int), and the one scalar
// f = ior_inv_eta * ior_inv_eta * (1 - F_i) * (1 - F_o), the products left to right
static S4 plastic_diffuse(const msk_bsdf_desc &b, float fdr_int, S4 rho, float F_i, float cos_o) {
    const float F_o = fresnel_F(cos_o, b.ior_eta);
    S4 D;
    if (b.sample_visible != 0) { for (int i = 0; i < 4; ++i) D.v[i] = rho.v[i] / (1.f - fdr_int * rho.v[i]); }      // the word is read as `nonlinear`
    else D = rho / (1.f - fdr_int);
    const float f = ((b.ior_inv_eta * b.ior_inv_eta) * (1.f - F_i)) * (1.f - F_o);
    return D * f;
}
// eval and pdf of type 6: the diffuse lobe's alone, for cos_i > 0 and cos_o > 0
static void plastic_eval_pdf(const Scene &sc, const msk_bsdf_desc &b, Scene::PlasticK k, Reflectance refl, V3 wi, V3 wo, S4 wl, S4 *val, float *pdf) {
    *val = s4(0.f); *pdf = 0.f;
    float F_i, ps, pd;
    if (!plastic_lobes(b, k.ssw, wi.z, &F_i, &ps, &pd) || !(wo.z > 0.f)) return;
    *val = (plastic_diffuse(b, k.fdr_int, reflectance_eval(sc, refl, wl), F_i, wo.z) * kInvPi) * wo.z;
    *pdf = pd * (kInvPi * wo.z);
}
// sample of type 6: sample1 < ps takes the delta coat, otherwise the diffuse base
static S4 plastic_sample(const Scene &sc, const msk_bsdf_desc &b, Scene::PlasticK k, Reflectance refl, V3 wi, float sample1, V2 sample, S4 wl, BSDFSampleRec *bs) {
    float F_i, ps, pd;
    if (!plastic_lobes(b, k.ssw, wi.z, &F_i, &ps, &pd)) return s4(0.f);
    bs->eta = 1.f;
    if (sample1 < ps) {
        bs->wo = mk3(-wi.x, -wi.y, wi.z);
        bs->pdf = ps;
        bs->sampled_type = kDeltaReflection;                          // D19: the mark of this sample, not of the entry
        return (spectrum_eval(sc, b.specular_reflectance, wl) * F_i) / ps;
    }
    bs->wo = square_to_cosine_hemisphere(sample);
    bs->pdf = pd * (kInvPi * bs->wo.z);
    bs->sampled_type = kDiffuseReflection;
    if (!(bs->pdf > 0.f)) return s4(0.f);
    return plastic_diffuse(b, k.fdr_int, reflectance_eval(sc, refl, wl), F_i, bs->wo.z) / pd;
}
// eval and pdf of type 7, the mixture: value(l) = s(l) * c + base(l), pdf = ps * p_s + pd * ((1 / pi) * cos_o)
static void roughplastic_eval_pdf(const Scene &sc, const msk_bsdf_desc &b, Scene::PlasticK k, Reflectance refl, V3 wi, V3 wo, S4 wl, S4 *val, float *pdf) {
    *val = s4(0.f); *pdf = 0.f;
    float F_i, ps, pd;
    if (!plastic_lobes(b, k.ssw, wi.z, &F_i, &ps, &pd) || !(wo.z > 0.f)) return;
    const float a = clamp_alpha(b.alpha_u);
    const S4 base = (plastic_diffuse(b, k.fdr_int, reflectance_eval(sc, refl, wl), F_i, wo.z) * kInvPi) * wo.z;
    const float pdf_d = pd * (kInvPi * wo.z);
    const V3 H = normalized(wo + wi);
    const float D = distr_eval(H, a, a);
    const float G = smith_g1(wi, H, a, a) * smith_g1(wo, H, a, a);
    const float F_h = fresnel_F(dot(wi, H), b.ior_eta);
    const float c = ((F_h * D) * G) / (4.f * wi.z);
    *val = spectrum_eval(sc, b.specular_reflectance, wl) * c + base;
    const float p_s = D == 0.f ? 0.f : (D * H.z) / (4.f * dot(wo, H));
    *pdf = ps * p_s + pdf_d;
}
// sample of type 7: a direction from the coat (sample_ggx, mirrored) or from the base, then eval / pdf of the mixture; never delta
static S4 roughplastic_sample(const Scene &sc, const msk_bsdf_desc &b, Scene::PlasticK k, Reflectance refl, V3 wi, float sample1, V2 sample, S4 wl, BSDFSampleRec *bs) {
    float F_i, ps, pd;
    if (!plastic_lobes(b, k.ssw, wi.z, &F_i, &ps, &pd)) return s4(0.f);
    bs->eta = 1.f;
    if (sample1 < ps) {
        const float a = clamp_alpha(b.alpha_u);
        float pm;
        const V3 m = sample_ggx(sample, a, a, &pm);
        bs->wo = m * 2.f * dot(wi, m) - wi;
        bs->sampled_type = kGlossyReflection;
        if (pm == 0.f || !(bs->wo.z > 0.f)) { bs->pdf = 0.f; return s4(0.f); }      // a direction was produced: value 0, pdf 0
    } else {
        bs->wo = square_to_cosine_hemisphere(sample);
        bs->sampled_type = kDiffuseReflection;
    }
    S4 val;
    roughplastic_eval_pdf(sc, b, k, refl, wi, bs->wo, wl, &val, &bs->pdf);
    return bs->pdf > 0.f ? val / bs->pdf : s4(0.f);
}

// one-sided evaluation (wi already on the front side for twosided); refl = reflectance_at() of the hit
static void bsdf_eval_pdf(const Scene &sc, const msk_bsdf_desc &b, Reflectance refl, V3 wi, V3 wo, S4 wl, S4 *val, float *pdf) {
    *val = s4(0.f); *pdf = 0.f;
    float cos_i = wi.z, cos_o = wo.z;
    if (b.type == MSK_BSDF_DIFFUSE) {                                  // diffuse.cpp:35-57
        if (cos_i > 0.f && cos_o > 0.f) {
            *val = reflectance_eval(sc, refl, wl) * kInvPi * cos_o;
            *pdf = square_to_cosine_hemisphere_pdf(wo);
        }
        return;
    }
    if (b.type == MSK_BSDF_ROUGHDIELECTRIC) { roughdielectric_eval_pdf(sc, b, wi, wo, wl, val, pdf); return; }
    if (b.type == MSK_BSDF_DIELECTRIC) return;                         // dielectric.cpp:74-82: eval and pdf are zero
    if (b.type == MSK_BSDF_CONDUCTOR) return;                          // msk_gpu.h at MSK_BSDF_CONDUCTOR: eval and pdf are zero
    if (is_plastic(b)) {
        Scene::PlasticK k;
        if (!plastic_k_of(sc, b, &k)) return;                          // a bare descriptor has no constants: zero, never another type's code
        if (b.type == MSK_BSDF_PLASTIC) plastic_eval_pdf(sc, b, k, refl, wi, wo, wl, val, pdf);
        else roughplastic_eval_pdf(sc, b, k, refl, wi, wo, wl, val, pdf);
        return;
    }
    if (b.type != MSK_BSDF_ROUGHCONDUCTOR) return;                     // no unknown type reaches the conductor's code (scene creation refuses them)
    const float au = clamp_alpha(b.alpha_u), av = clamp_alpha(b.alpha_v);
    // roughconductor.cpp:82-98 eval
    if (cos_i > 0.f && cos_o > 0.f) {
        V3 H = normalized(wo + wi);
        float D = distr_eval(H, au, av);
        if (D != 0) {
            float G = smith_g1(wi, H, au, av) * smith_g1(wo, H, au, av);
            float result = D * G / (4.f * wi.z);
            S4 F = fresnel_conductor4(dot(wi, H), spectrum_eval(sc, b.eta, wl), spectrum_eval(sc, b.k, wl));
            *val = F * spectrum_eval(sc, b.specular_reflectance, wl) * result;
        }
    }
    // roughconductor.cpp:100-117 pdf
    V3 m = normalized(wo + wi);
    if (cos_i > 0.f && cos_o > 0.f && dot(wi, m) > 0.f && dot(wo, m) > 0.f) {
        if (b.sample_visible) *pdf = distr_eval(m, au, av) * smith_g1(wi, m, au, av) / (4.f * cos_i);
        else *pdf = (distr_eval(m, au, av) * m.z) / (4.f * dot(wo, m));
    }
}
static S4 bsdf_sample(const Scene &sc, const msk_bsdf_desc &b, Reflectance refl, V3 wi, float sample1, V2 sample, S4 wl, BSDFSampleRec *bs) {
    bs->wo = mk3(0, 0, 0); bs->pdf = 0.f; bs->eta = 1.f; bs->sampled_type = 0;       // render/bsdf.h:75-77
    if (b.type == MSK_BSDF_ROUGHDIELECTRIC) return roughdielectric_sample(sc, b, wi, sample1, sample, wl, bs);
    if (b.type == MSK_BSDF_DIELECTRIC) return dielectric_sample(sc, b, wi, sample, wl, bs);
    if (b.type == MSK_BSDF_CONDUCTOR) return conductor_sample(sc, b, wi, wl, bs);
    if (is_plastic(b)) {
        Scene::PlasticK k;
        if (!plastic_k_of(sc, b, &k)) return s4(0.f);
        return b.type == MSK_BSDF_PLASTIC ? plastic_sample(sc, b, k, refl, wi, sample1, sample, wl, bs) : roughplastic_sample(sc, b, k, refl, wi, sample1, sample, wl, bs);
    }
    if (b.type != MSK_BSDF_DIFFUSE && b.type != MSK_BSDF_ROUGHCONDUCTOR) return s4(0.f);      // no unknown type reaches the conductor's code
    float cos_i = wi.z;
    if (cos_i <= 0.f) return s4(0.f);
    if (b.type == MSK_BSDF_DIFFUSE) {                                  // diffuse.cpp:18-33
        bs->wo = square_to_cosine_hemisphere(sample);
        bs->pdf = square_to_cosine_hemisphere_pdf(bs->wo);
        bs->sampled_type = kDiffuseReflection;
        return bs->pdf > 0.f ? reflectance_eval(sc, refl, wl) : s4(0.f);
    }
    // roughconductor.cpp:52-80
    const float au = clamp_alpha(b.alpha_u), av = clamp_alpha(b.alpha_v);
    V3 m = sample_ggx(sample, au, av, &bs->pdf);
    bs->wo = m * 2.f * dot(wi, m) - wi;                                // fresnel.h:17-21 reflect(wi, m)
    bs->sampled_type = kGlossyReflection;
    if (!(bs->pdf != 0.f && bs->wo.z > 0.f)) return s4(0.f);
    float weight;
    if (b.sample_visible) weight = smith_g1(bs->wo, m, au, av);
    else weight = smith_g1(wi, m, au, av) * smith_g1(bs->wo, m, au, av) * dot(wi, m) / (cos_i * m.z);
    bs->pdf /= 4.f * dot(bs->wo, m);
    S4 F = fresnel_conductor4(dot(wi, m), spectrum_eval(sc, b.eta, wl), spectrum_eval(sc, b.k, wl));
    return F * weight;
}
// twosided.cpp:38-101: pick the nested BSDF by the side wi is on, flip z of wi and wo on the back
static const msk_bsdf_desc *bsdf_side(const Scene &sc, const msk_bsdf_desc &b, V3 *wi, bool *flipped) {
    *flipped = false;
    if (b.back_bsdf >= 0 && wi->z < 0.f) { wi->z *= -1.f; *flipped = true; return &sc.bsdfs[b.back_bsdf]; }
    return &b;
}

struct Counters { uint64_t samples = 0, segments = 0, shadow_rays = 0, invalid = 0; };

// what a ray that leaves the scene in direction d sees: the constant sky's radiance, or the image's L(d) (msk_gpu.h at msk_envmap_desc)
static S4 environment_radiance(const Scene &sc, V3 d, S4 wl) {
    if (!sc.env_is_image) return emitter_radiance(sc, sc.env, wl);
    float sin_theta;
    return env_radiance(sc, env_dir_to_uv(sc.envmap, d, &sin_theta), wl);
}

// ===========================================================================
// a5  PathTracer::sample (integrators/path.cpp:23-125) with a11 diffuse BSDF
//     (bsdfs/diffuse.cpp:18-57) inlined where the reference makes virtual calls
// ===========================================================================
static S4 path_sample(const Scene &sc, Sampler &sampler, Ray ray, S4 wl, const msk_render_params &prm,
                      Counters &cnt) {
    const int max_depth = prm.max_depth, rr_depth = prm.rr_depth;
    const bool hide_emitter = prm.hide_emitters != 0;
    S4 throughput = s4(1.f), result = s4(0.f);
    float eta = 1.f;
    bool scattered = false;
    ++cnt.segments;
    Interaction si = compute_interaction(sc, ray, closest_hit(sc, ray));
    for (int depth = 1; depth <= max_depth || max_depth < 0; depth++) {
        if (!si.valid()) {                                         // path.cpp:34-41
            if (depth == 1 && (!hide_emitter || scattered) && sc.env >= 0)
                result = result + throughput * environment_radiance(sc, ray.d, wl);
            break;
        }
        int emitter = sc.meshes[si.mesh].emitter_id;
        if (emitter >= 0 && depth == 1 && (!hide_emitter || scattered))
            result = result + throughput * emitter_eval(sc, emitter, si, wl);
        if (depth >= max_depth && max_depth > 0) break;
        const uint32_t base = 3 + 3 * (uint32_t) (depth - 1);
        const int bsdf_id = sc.meshes[si.mesh].bsdf_id;
        const msk_bsdf_desc &bsdf = sc.bsdfs[bsdf_id];
        // msk_gpu.h at msk_mask_desc: the opacity of the entry the mesh names, before the twosided flip; in a scene that holds a
        // mask every entry has one (1 without a mask, where u.x / 1 and 1 * pdf are exact)
        const bool masked = sc.any_mask;
        const float opacity = masked ? mask_opacity(sc, bsdf_id, si.uv) : 1.f;
        // ---- direct illumination (path.cpp:56-67): only for a BSDF with a Smooth lobe.  Without one the sample is not drawn
        // (MSK_RNG_PCG_BLOCK: no next2d(); MSK_RNG_COUNTER: the pair base + 0 stays unused) and `ds` stays default-constructed
        DirectSample ds; ds.pdf = 0; ds.emitter = -1;
        bool has_shadow = false;               // (tallies only) this bounce's next-event term is not zero: the device traces its shadow ray
        if (bsdf_has_smooth_lobe(bsdf)) {
            V2 u; sampler.pair(base + 0, &u.x, &u.y);
            S4 emitter_val, unoccluded = s4(0.f);
            bool occluded = false;
            ds = sample_emitter_direct(sc, si, u, wl, &emitter_val, &cnt.shadow_rays, &unoccluded, &occluded);
            if (ds.falloff) tally(ds.falloff == 1 ? kTallySpotBeam : ds.falloff == 2 ? kTallySpotRamp : kTallySpotDark);
            if (ds.pdf != 0.f) {
                V3 wo = si.sh.to_local(ds.d), wi_s = si.wi;
                bool flipped;
                const msk_bsdf_desc *bb = bsdf_side(sc, bsdf, &wi_s, &flipped);
                if (flipped) wo.z *= -1.f;
                S4 bsdf_val; float bsdf_pdf;
                bsdf_eval_pdf(sc, *bb, reflectance_at(sc, *bb, si.uv), wi_s, wo, wl, &bsdf_val, &bsdf_pdf);
                if (masked) { bsdf_val = bsdf_val * opacity; bsdf_pdf = opacity * bsdf_pdf; }      // eval = a eval_X, pdf = a pdf_X
                // D14: a delta emitter cannot be reached by a BSDF sample: weight 1
                float weight = ds.point ? 1.f : mis_weight(ds.pdf, bsdf_pdf);
                {
                    const S4 term = throughput * unoccluded * bsdf_val * weight;
                    if (term.v[0] != 0.f || term.v[1] != 0.f || term.v[2] != 0.f || term.v[3] != 0.f) { has_shadow = true; tally(kTallyShadowNonzero); }
                    if (ds.point) tally(occluded ? kTallyPointOccluded : kTallyPointUnoccluded);
                    const int32_t etype = sc.emitters[ds.emitter].type;
                    if (etype == MSK_EMITTER_SPOT) tally(occluded ? kTallySpotOccluded : kTallySpotUnoccluded);
                    if (etype == MSK_EMITTER_DIRECTIONAL) tally(occluded ? kTallySunOccluded : kTallySunUnoccluded);
                }
                if (g_trace_path)
                    std::printf("  d%d NEE: ds.pdf %.9g bsdf_pdf %.9g w %.9g emitter_val %.9g bsdf_val %.9g %.9g %.9g %.9g thr %.9g wo_local %.9g %.9g %.9g wi %.9g %.9g %.9g\n", depth, ds.pdf,
                                bsdf_pdf, weight, emitter_val.v[0], bsdf_val.v[0], bsdf_val.v[1], bsdf_val.v[2], bsdf_val.v[3], throughput.v[0], wo.x, wo.y, wo.z, wi_s.x, wi_s.y, wi_s.z);
                result = result + throughput * emitter_val * bsdf_val * weight;
            }
        }
        // ---- BSDF sampling (path.cpp:71-73), D3 order
        float sample1 = sampler.single(base + 1, 0);
        V2 u2; sampler.pair(base + 2, &u2.x, &u2.y);
        BSDFSampleRec bs;
        S4 bsdf_val;
        // mask.cpp:43-44: the lobe is picked by u.x; u.x < a: X with u.x / a, else the null lobe (pdf = 1 - a, value 1, eta = 1, delta)
        bool null_lobe = false;
        if (masked) { null_lobe = !(u2.x < opacity); if (!null_lobe) u2.x = u2.x / opacity; }
        if (null_lobe) {
            bs.wo = mk3(0.f, 0.f, 0.f); bs.pdf = 1.f - opacity; bs.eta = 1.f; bs.sampled_type = kNull;
            bsdf_val = s4(1.f);
            tally(kTallyNullLobe);
        } else {
            V3 wi_s = si.wi; bool flipped;
            const msk_bsdf_desc *bb = bsdf_side(sc, bsdf, &wi_s, &flipped);
            bsdf_val = bsdf_sample(sc, *bb, reflectance_at(sc, *bb, si.uv), wi_s, sample1, u2, wl, &bs);
            if (flipped) bs.wo.z *= -1.f;
            if (masked) bs.pdf = opacity * bs.pdf;                 // D16: pdf = a pdf_X, the value stays X's
            if (is_plastic(*bb)) {                                 // (tallies only)
                if (flipped) tally(kTallyPlasticBackFace);
                if (bb->back_bsdf < 0 && !(wi_s.z > 0.f)) tally(kTallyPlasticFromBehind);
                if (bb->type == MSK_BSDF_PLASTIC) { if (bs.sampled_type == kDeltaReflection) tally(kTallyPlasticCoat); else if (bs.sampled_type) tally(kTallyPlasticBase); }
                else if (bs.sampled_type == kGlossyReflection) tally(bs.pdf == 0.f ? kTallyRoughPlasticFailed : kTallyRoughPlasticCoat);
                else if (bs.sampled_type) tally(kTallyRoughPlasticBase);
            }
        }
        if (null_lobe && is_plastic(bsdf)) tally(kTallyNullOverPlastic);
        const bool coat_sample = !null_lobe && is_plastic(bsdf) && (bs.sampled_type == kDeltaReflection || bs.sampled_type == kGlossyReflection);
        const V3 bs_wo = bs.wo; const float bs_pdf = bs.pdf, bs_eta = bs.eta;
        const uint32_t sampled_type = bs.sampled_type;
        {   // (tallies only) where the device's segment count parts from `if (sampled_type) ++cnt.segments` below
            const S4 next = throughput * bsdf_val;
            const bool dead = !(next.v[0] != 0.f || next.v[1] != 0.f || next.v[2] != 0.f || next.v[3] != 0.f);
            if (!sampled_type || dead) tally(kTallyDeadSample);
            if (sampled_type && dead && !has_shadow) tally(kTallySegmentDropped);
            if (!sampled_type && has_shadow) tally(kTallySegmentExtra);
        }
        // path.cpp:73: sampled_type (0 on failure) != Null is true for every sample but a mask's null lobe
        if (!null_lobe) scattered = true;
        // D18: under hide_emitters an emitter of any kind reached while `scattered` is false adds nothing (only a mask's null lobe
        // leaves it false after a bounce).  "Adds nothing", not path.cpp:92-93's `break`: a null bounce takes Russian roulette like
        // any other (msk_gpu.h at msk_mask_desc), so MSK_RNG_PCG_BLOCK draws that number before the path ends on the miss.
        const bool hidden = hide_emitter && !scattered;
        // the null lobe: the incoming ray's own world direction, bit for bit (no frame round trip)
        V3 wo = null_lobe ? ray.d : si.sh.to_world(bs_wo);
        bool hit_emitter = false, env_hit = false;
        S4 value = s4(0.f);
        ray = Ray{si.p, wo, (1.f + max_abs(si.p)) * kRayEpsilon, kInf};   // interaction.h:40-44
        if (sampled_type) ++cnt.segments;     // statistics only: the zero-direction ray of a failed sample is not counted
        Interaction si_bsdf = compute_interaction(sc, ray, closest_hit(sc, ray));
        if (si_bsdf.valid()) {
            int em = sc.meshes[si_bsdf.mesh].emitter_id;
            if (em >= 0) {
                value = emitter_eval(sc, em, si_bsdf, wl);
                // records.cpp:7-14 set_query
                ds.p = si_bsdf.p; ds.n = si_bsdf.sh.n; ds.emitter = em; ds.d = ray.d; ds.dist = si_bsdf.t; ds.point = false;
                hit_emitter = true;
            }
        } else if (sc.env >= 0) {                                  // path.cpp:90-95
            value = environment_radiance(sc, ray.d, wl);
            hit_emitter = env_hit = true;  // `ds` is NOT re-queried: D9's MIS weight below uses the NEE sample's record (but D12, D15)
        } else {
            break;                                                 // path.cpp:96-97
        }
        throughput = throughput * bsdf_val;
        if (g_trace_path)
            std::printf("  d%d sample: bsdf %d type %u wo %.9g %.9g %.9g pdf %.9g weight %.9g %.9g %.9g %.9g -> thr %.9g %.9g %.9g %.9g hit %d t %.9g emitter %d\n", depth,
                        (int) sc.meshes[si.mesh].bsdf_id, sampled_type, bs_wo.x, bs_wo.y, bs_wo.z, bs_pdf, bsdf_val.v[0], bsdf_val.v[1], bsdf_val.v[2], bsdf_val.v[3],
                        throughput.v[0], throughput.v[1], throughput.v[2], throughput.v[3], (int) si_bsdf.valid(), si_bsdf.t, (int) hit_emitter);
        eta *= bs_eta;
        if (hit_emitter) {
            // path.cpp:104-106: a delta lobe has no emitter pdf (and after one `ds` may hold no emitter at all); "the last bounce
            // was delta" holds when the null lobe was taken or X is delta (msk_gpu.h at msk_mask_desc)
            const bool delta = (sampled_type & (kDelta | kNull)) != 0u || !bsdf_has_smooth_lobe(bsdf);
            const size_t n_em = sc.emitters.size();
            float emitter_pdf = 0.f;
            if (delta) emitter_pdf = 0.f;
            else if (env_hit && sc.env_is_image) {                 // D12: the density of the ray's own direction
                float sin_theta;
                const V2 uv = env_dir_to_uv(sc.envmap, ray.d, &sin_theta);
                emitter_pdf = env_pdf(sc.envmap, uv, sin_theta);
                if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
            } else if (env_hit && sc.own_density_sky) {            // D15
                emitter_pdf = kInvFourPi;
                if (n_em != 1) emitter_pdf = emitter_pdf * (1.f / n_em);
                tally(kTallySkyOwnDensity);
            } else emitter_pdf = pdf_emitter_direct(sc, ds);
            const float weight = mis_weight(bs_pdf, emitter_pdf);
            if (null_lobe) tally(kTallyEmitterAfterNull);
            if (sampled_type & kDelta) tally(kTallyEmitterAfterDelta);
            if ((sampled_type & kDelta) && bsdf.type == MSK_BSDF_PLASTIC) tally(kTallyEmitterAfterCoat);
            if (env_hit && sc.env_is_image && !delta && weight > 0.f && weight < 1.f) tally(kTallyEnvmapMissSmooth);
            if (hidden) { if (!env_hit) tally(kTallyAreaHidden); }
            else result = result + throughput * value * weight;
        }
        si = si_bsdf;
        if (depth + 1 >= rr_depth) {                               // path.cpp:116-122
            float q = std::min(max4(throughput) * eta * eta, 0.95f);
            if (sampler.single(base + 1, 1) >= q) { if (null_lobe) tally(kTallyRRAfterNull); if (coat_sample) tally(kTallyRRAfterCoat); break; }
            throughput = throughput / q;
        }
    }
    return result;
}

// ===========================================================================
// The `direct` integrator: include/msk_gpu.h at msk_direct_params, DESIGN.md section 9.  One primary ray, N light samples and M
// BSDF samples at its hit; the fp32 operation order of a term is the header's.  rr_depth and max_depth are not read.
// ===========================================================================
static inline bool any_nonzero(S4 v) { return v.v[0] != 0.f || v.v[1] != 0.f || v.v[2] != 0.f || v.v[3] != 0.f; }
// the power heuristic over the sample counts
static float direct_weight(float n_a, float p_a, float n_b, float p_b) {
    float a = n_a * p_a, b = n_b * p_b;
    a = a * a; b = b * b;
    return a > 0.f ? a / (a + b) : 0.f;
}
// what msk_oracle_direct_terms reports of one camera sample: every factor of every term, before the weights and the counts
struct DirectLightTerm { uint32_t pair = 0; int emitter = -1; float p_l = 0.f, p_b = 0.f; bool point = false, shadow = false, occluded = false; S4 prod; };
struct DirectBsdfTerm { uint32_t pair_lobe = 0, pair_dir = 0; float p_b = 0.f, p_e = 0.f; bool traced = false, reached = false, escaped = false; S4 prod; };
struct DirectTerms { bool hit = false; S4 emission; std::vector<DirectLightTerm> light; std::vector<DirectBsdfTerm> bsdf; };

static S4 direct_sample(const Scene &sc, Sampler &sampler, Ray ray, S4 wl, const msk_render_params &prm, uint32_t N, uint32_t M,
                        Counters &cnt, DirectTerms *terms = nullptr) {
    const bool hide_emitter = prm.hide_emitters != 0;
    const float fN = (float) N, fM = (float) M;
    const size_t n_em = sc.emitters.size();
    S4 result = s4(0.f);
    ++cnt.segments;
    const Interaction si = compute_interaction(sc, ray, closest_hit(sc, ray));
    if (terms) { terms->hit = si.valid(); terms->emission = s4(0.f); }
    // ---- emission: the environment behind a primary miss, the front of an emitter at the primary hit; hide_emitters removes both
    if (!si.valid()) {
        if (!hide_emitter && sc.env >= 0) {
            const S4 e = environment_radiance(sc, ray.d, wl);
            if (terms) terms->emission = e;
            result = result + e;
            tally(kDirPrimaryMissEnv);
        }
        return result;
    }
    const int emitter = sc.meshes[si.mesh].emitter_id;
    if (emitter >= 0) {
        if (!hide_emitter) {
            const S4 e = emitter_eval(sc, emitter, si, wl);
            if (terms) terms->emission = e;
            result = result + e;
            tally(kDirPrimaryEmitterSeen);
        } else tally(kDirPrimaryEmitterHidden);
    }
    const msk_bsdf_desc &bsdf = sc.bsdfs[sc.meshes[si.mesh].bsdf_id];
    V3 wi_s = si.wi;
    bool flipped;
    const msk_bsdf_desc *bb = bsdf_side(sc, bsdf, &wi_s, &flipped);
    if (flipped) tally(kDirTwosidedFlipped);
    const Reflectance refl = reflectance_at(sc, *bb, si.uv);
    const bool smooth = bsdf_has_smooth_lobe(bsdf);
    // ---- light samples: pair 3 + i; none at a BSDF without a smooth lobe, none without an emitter
    if (!smooth && N > 0 && n_em > 0) tally(kDirLightSkippedDelta);
    if (smooth && n_em > 0)
        for (uint32_t i = 0; i < N; ++i) {
            V2 u; sampler.pair(3u + i, &u.x, &u.y);
            DirectLightTerm lt;
            if (terms) lt.pair = sampler.log ? sampler.log->back() : 3u + i;
            S4 emitter_val, unoccluded = s4(0.f);
            bool occluded = false;
            uint64_t traced_by_block = 0;       // (the building block counts a ray per non-zero density; this integrator counts by the term)
            const DirectSample ds = sample_emitter_direct(sc, si, u, wl, &emitter_val, &traced_by_block, &unoccluded, &occluded);
            lt.emitter = ds.emitter; lt.p_l = ds.pdf; lt.point = ds.point; lt.prod = s4(0.f);
            if (ds.emitter >= 0 && n_em > 1 && (size_t) ds.emitter == n_em - 1) tally(kDirLightLastEmitter);
            const int etype = ds.emitter >= 0 ? (int) sc.emitters[ds.emitter].type : -1;
            if (etype == MSK_EMITTER_CONSTANT) tally(kDirLightConstantSky);
            if (etype == MSK_EMITTER_ENVMAP) tally(kDirLightImage);
            if (etype == MSK_EMITTER_AREA && ds.pdf == 0.f) tally(kDirLightAreaBack);
            if (ds.falloff == 3) tally(kDirLightSpotDark);
            if (ds.pdf != 0.f) {
                V3 wo = si.sh.to_local(ds.d);
                if (flipped) wo.z *= -1.f;
                S4 bsdf_val; float bsdf_pdf;
                bsdf_eval_pdf(sc, *bb, refl, wi_s, wo, wl, &bsdf_val, &bsdf_pdf);
                const float w_l = ds.point ? 1.f : direct_weight(fN, ds.pdf, fM, bsdf_pdf);      // a delta light: weight 1
                const S4 prod = unoccluded * bsdf_val;
                S4 term = prod * w_l;
                lt.p_b = bsdf_pdf; lt.prod = prod;
                if (any_nonzero(term)) {                                  // the shadow ray: an occluded sample adds nothing
                    ++cnt.shadow_rays;
                    lt.shadow = true; lt.occluded = occluded;
                    if (ds.point) tally(occluded ? kDirLightPointOccluded : kDirLightPointVisible);
                    if (etype == MSK_EMITTER_SPOT) tally(occluded ? kDirLightSpotOccluded : kDirLightSpotVisible);
                    if (etype == MSK_EMITTER_DIRECTIONAL) tally(occluded ? kDirLightSunOccluded : kDirLightSunVisible);
                    if (etype == MSK_EMITTER_POINT) tally(occluded ? kDirLightPointOnlyOccluded : kDirLightPointOnlyVisible);
                    if (etype == MSK_EMITTER_AREA) tally(occluded ? kDirLightAreaOccluded : kDirLightAreaVisible);
                    if (!occluded) {
                        term = term / fN;
                        result = result + term;
                    }
                }
            }
            if (terms) terms->light.push_back(lt);
        }
    // ---- BSDF samples: pair 3 + N + 2 j the lobe choice (.x), the next pair the direction
    for (uint32_t j = 0; j < M; ++j) {
        const uint32_t base = 3u + N + 2u * j;
        DirectBsdfTerm bt;
        const float sample1 = sampler.single(base, 0);
        if (terms) bt.pair_lobe = sampler.log ? sampler.log->back() : base;
        V2 u2; sampler.pair(base + 1u, &u2.x, &u2.y);
        if (terms) bt.pair_dir = sampler.log ? sampler.log->back() : base + 1u;
        BSDFSampleRec bs;
        const S4 bsdf_val = bsdf_sample(sc, *bb, refl, wi_s, sample1, u2, wl, &bs);
        if (flipped) bs.wo.z *= -1.f;
        bt.p_b = bs.pdf; bt.prod = s4(0.f);
        if (bs.sampled_type && any_nonzero(bsdf_val)) {
            ++cnt.segments;
            bt.traced = true;
            const Ray r2{si.p, si.sh.to_world(bs.wo), (1.f + max_abs(si.p)) * kRayEpsilon, kInf};
            const Interaction sb = compute_interaction(sc, r2, closest_hit(sc, r2));
            const bool delta = (bs.sampled_type & kDelta) != 0u || !smooth;
            S4 value = s4(0.f);
            float p_e = 0.f;
            bool reached = false;
            bt.escaped = !sb.valid();
            if (sb.valid()) {
                const int em = sc.meshes[sb.mesh].emitter_id;
                if (em >= 0) {
                    value = emitter_eval(sc, em, sb, wl);
                    DirectSample q;                                       // records.cpp:7-14 set_query
                    q.p = sb.p; q.n = sb.sh.n; q.emitter = em; q.d = r2.d; q.dist = sb.t; q.pdf = 0.f;
                    p_e = pdf_emitter_direct(sc, q);
                    reached = true;
                    if (!(sb.wi.z > 0.f)) tally(kDirBsdfEmitterBack);
                } else tally(kDirBsdfNonEmitter);
            } else if (sc.env >= 0 && sc.env_is_image) {                  // value and density of the ray's own direction
                float sin_theta;
                const V2 uv = env_dir_to_uv(sc.envmap, r2.d, &sin_theta);
                value = env_radiance(sc, uv, wl);
                p_e = env_pdf(sc.envmap, uv, sin_theta);
                if (n_em != 1) p_e = p_e * (1.f / n_em);
                reached = true;
                tally(kDirBsdfMissImage);
            } else if (sc.env >= 0) {                                     // the `constant` sky: its own density, always
                value = emitter_radiance(sc, sc.env, wl);
                p_e = kInvFourPi;
                if (n_em != 1) p_e = p_e * (1.f / n_em);
                reached = true;
                tally(kDirBsdfMissConstant);
            } else tally(kDirBsdfMissNothing);
            if (delta) p_e = 0.f;
            if (reached) {
                const float w_b = direct_weight(fM, bs.pdf, fN, p_e);
                const S4 prod = bsdf_val * value;
                S4 term = prod * w_b;
                term = term / fM;
                result = result + term;
                bt.reached = true; bt.p_e = p_e; bt.prod = prod;
                if (delta) tally(kDirBsdfEmitterAfterDelta);
                else if (sb.valid() && sb.wi.z > 0.f && w_b > 0.f && w_b < 1.f) tally(kDirBsdfEmitterFrontMis);
            }
        } else tally(kDirBsdfNotTraced);
        if (terms) terms->bsdf.push_back(bt);
    }
    return result;
}
// what the library refuses of a `direct` call (msk_gpu.h): 0 when it is taken
// D24: a lens scene under MSK_RNG_PCG_BLOCK (the reference's sampler draws no aperture sample that could pin that mode)
static int lens_refusal(const Scene &sc, const msk_render_params &prm) {
    return sc.has_lens && prm.rng_mode != MSK_RNG_COUNTER ? MSK_ERR_UNSUPPORTED : 0;
}
static int direct_refusal(const Scene &sc, const msk_render_params &prm, const msk_direct_params &dp) {
    if (sc.any_mask) return MSK_ERR_UNSUPPORTED;
    if (sc.any_plastic) return MSK_ERR_UNSUPPORTED;                    // D22: as msk_gpu_render_direct does
    if (prm.rng_mode != MSK_RNG_COUNTER) return MSK_ERR_UNSUPPORTED;
    if (dp.light_samples > 4096u || dp.bsdf_samples > 4096u || (dp.light_samples == 0u && dp.bsdf_samples == 0u)) return MSK_ERR_INVALID_ARG;
    return 0;
}

// ===========================================================================
// a14/a15  ImageBlock (imageblock.cpp:9-173) and a1 BlockGenerator (:176-247)
// ===========================================================================
struct ImageBlock {
    int off_x = 0, off_y = 0, size_x = 0, size_y = 0, border = 0, channels = 5;
    std::vector<float> data;
    float radius = 0, scale_factor = 0; const float *lut = nullptr;
    bool warn_negative = true, warn_invalid = true;                     // imageblock.h:16
    uint64_t invalid = 0;                                               // how often put() would have logged "Invalid sample value"
    void init(int sx, int sy, const msk_film_desc *filter, bool with_border) {
        if (filter) {
            radius = filter->filter_radius; lut = filter->filter_lut;
            scale_factor = float(MSK_FILTER_RESOLUTION) / radius;        // rfilter.cpp:21
            border = with_border ? (int) std::ceil(radius - .5f) : 0;     // rfilter.cpp:22
        }
        size_x = sx; size_y = sy;
        data.assign((size_t) channels * (sx + 2 * border) * (sy + 2 * border), 0.f);
    }
    float eval_discretized(float x) const {                             // rfilter.h:13-16
        return lut[std::min((int) std::fabs(x * scale_factor), MSK_FILTER_RESOLUTION)];
    }
    void put(V2 pos_, const float *value) {                             // imageblock.cpp:55-114
        if (warn_negative || warn_invalid) {                            // :57-81 — the sample is warned about and splatted all the same
            bool is_valid = true;
            if (warn_negative) for (int k = 0; k < channels; ++k) is_valid &= value[k] >= -1e-5f;
            if (warn_invalid) for (int k = 0; k < channels; ++k) is_valid &= (bool) std::isfinite(value[k]);
            if (!is_valid) ++invalid;
        }
        int sx = size_x + 2 * border, sy = size_y + 2 * border;
        const V2 pos{pos_.x - 0.5f - (off_x - border), pos_.y - 0.5f - (off_y - border)};
        int lo_x = std::max((int) std::ceil(pos.x - radius), 0), lo_y = std::max((int) std::ceil(pos.y - radius), 0);
        int hi_x = std::min((int) std::floor(pos.x + radius), sx - 1),
            hi_y = std::min((int) std::floor(pos.y + radius), sy - 1);
        float wx[16], wy[16];
        for (int x = lo_x, idx = 0; x <= hi_x; ++x) wx[idx++] = eval_discretized(x - pos.x);
        for (int y = lo_y, idx = 0; y <= hi_y; ++y) wy[idx++] = eval_discretized(y - pos.y);
        for (int y = lo_y, yr = 0; y <= hi_y; ++y, ++yr) {
            const float weight_y = wy[yr];
            float *dest = data.data() + ((size_t) y * sx + lo_x) * channels;
            for (int x = lo_x, xr = 0; x <= hi_x; ++x, ++xr) {
                const float weight = wx[xr] * weight_y;
                for (int k = 0; k < channels; ++k) *dest++ += weight * value[k];
            }
        }
    }
};
// imageblock.cpp:36-53 put(block) -> accumulate_2d (:133-173): source block with
// border into a borderless target at offset (0,0)
// film = HDRFilm's storage: a borderless ImageBlock of the crop size at the crop offset (hdrfilm.cpp:37-38; the whole film by default)
static void film_put(float *film, int fw, int fh, const ImageBlock &b, int crop_x = 0, int crop_y = 0) {
    int ssx = b.size_x + 2 * b.border, ssy = b.size_y + 2 * b.border;
    int tox = b.off_x - b.border - crop_x, toy = b.off_y - b.border - crop_y;   // source_offset - target_offset
    int sox = 0, soy = 0, szx = ssx, szy = ssy;
    int incx = std::max(0, std::max(-sox, -tox)), incy = std::max(0, std::max(-soy, -toy));
    sox += incx; soy += incy; tox += incx; toy += incy; szx -= incx; szy -= incy;
    int decx = std::max(0, std::max(sox + szx - ssx, tox + szx - fw)),
        decy = std::max(0, std::max(soy + szy - ssy, toy + szy - fh));
    szx -= decx; szy -= decy;
    if (szx <= 0 || szy <= 0) return;
    const size_t columns = (size_t) szx * b.channels;
    const float *src = b.data.data() + ((size_t) sox + (size_t) soy * ssx) * b.channels;
    float *dst = film + ((size_t) tox + (size_t) toy * fw) * b.channels;
    for (int y = 0; y < szy; ++y) {
        for (size_t i = 0; i < columns; ++i) dst[i] += src[i];
        src += (size_t) ssx * b.channels; dst += (size_t) fw * b.channels;
    }
}

struct BlockDesc { int off_x, off_y, size_x, size_y; };
// imageblock.cpp:176-247
static std::vector<BlockDesc> spiral_blocks(int w, int h, int block_size) {
    int bx = (int) std::ceil(w / (float) block_size), by = (int) std::ceil(h / (float) block_size);
    int count = bx * by;
    std::vector<BlockDesc> out;
    int dir = 0 /* Right, Down, Left, Up */, px = bx / 2, py = by / 2, steps_left = 1, steps = 1;
    for (int counter = 0; counter < count;) {
        int ox = px * block_size, oy = py * block_size;
        out.push_back(BlockDesc{ox, oy, std::min(w - ox, block_size), std::min(h - oy, block_size)});
        ++counter;
        if (counter != count) {
            do {
                switch (dir) { case 0: ++px; break; case 1: ++py; break; case 2: --px; break; case 3: --py; break; }
                if (--steps_left == 0) {
                    dir = (dir + 1) % 4;
                    if (dir == 2 || dir == 0) ++steps;
                    steps_left = steps;
                }
            } while (px < 0 || py < 0 || px >= bx || py >= by);
        }
    }
    return out;
}

// ===========================================================================
// a2  render_sample (integrator.cpp:103-126), returns the {X,Y,Z} handed to put
// ===========================================================================
struct AovSpec {
    std::vector<int32_t> types;
    int channels = 0;
    static int width(int32_t t) { static const int w[6] = {1, 3, 2, 3, 3, 4}; return t >= 0 && t < 6 ? w[t] : -1; }
};
// integrators/aov.cpp:87-144 (aov == nullptr: the plain "path" integrator); aovs receives spec.channels floats
static void render_sample(const Scene &sc, Sampler &sampler, V2 pos, const msk_render_params &prm,
                          Counters &cnt, V2 *position_sample, float xyz[3], const AovSpec *aov = nullptr, float *aovs = nullptr,
                          const msk_direct_params *direct = nullptr, DirectTerms *terms = nullptr, S4 *out_wl = nullptr, S4 *out_weight = nullptr,
                          S4 *out_spectral = nullptr) {
    float jx, jy; sampler.pair(0, &jx, &jy);
    *position_sample = V2{pos.x + jx, pos.y + jy};
    float wavelength_sample = sampler.single(1, 0);
    V2 aperture{0.5f, 0.5f};
    if (sampler.mode == MSK_RNG_PCG_BLOCK) { float a, b; sampler.pair(2, &a, &b); }   // aperture sample, unused (a lens scene is refused in this mode)
    else if (sc.has_lens) sampler.pair(2, &aperture.x, &aperture.y);                  // D24: pair 2 of the sample's key
    S4 wl, ray_weight;
    Ray ray = camera_ray(sc, wavelength_sample, *position_sample, &wl, &ray_weight, aperture, true);
    ++cnt.samples;
    S4 result;
    if (out_wl) *out_wl = wl;
    if (out_weight) *out_weight = ray_weight;
    if (direct) {                                                  // the "direct" integrator in place of "path"
        result = direct_sample(sc, sampler, ray, wl, prm, direct->light_samples, direct->bsdf_samples, cnt, terms);
        if (out_spectral) *out_spectral = result;
    } else if (!aov) {
        result = path_sample(sc, sampler, ray, wl, prm, cnt);
    } else {
        result = s4(0.f);                                          // aov.cpp:91 leaves it uninitialised without a nested integrator
        Interaction si = compute_interaction(sc, ray, closest_hit(sc, ray));   // aov.cpp:89
        const bool hit = si.valid();
        for (int32_t type : aov->types) {
            switch (type) {
                case MSK_AOV_DEPTH: *aovs++ = hit ? si.t : 0.f; break;
                case MSK_AOV_POSITION: *aovs++ = hit ? si.p.x : 0.f; *aovs++ = hit ? si.p.y : 0.f; *aovs++ = hit ? si.p.z : 0.f; break;
                case MSK_AOV_UV: *aovs++ = hit ? si.uv.x : 0.f; *aovs++ = hit ? si.uv.y : 0.f; break;
                case MSK_AOV_GEO_NORMAL: *aovs++ = hit ? si.n.x : 0.f; *aovs++ = hit ? si.n.y : 0.f; *aovs++ = hit ? si.n.z : 0.f; break;
                case MSK_AOV_SH_NORMAL: *aovs++ = hit ? si.sh.n.x : 0.f; *aovs++ = hit ? si.sh.n.y : 0.f; *aovs++ = hit ? si.sh.n.z : 0.f; break;
                case MSK_AOV_PATH_RGBA: {
                    S4 spec = path_sample(sc, sampler, ray, wl, prm, cnt);
                    float c[3]; spectrum_to_xyz(sc, spec, wl, c);
                    // core/spectrum.h:138-143 xyz_to_srgb (Eigen 3x3 * vector: a0 + (a1 + a2) per row)
                    *aovs++ = 3.240479f * c[0] + (-1.537150f * c[1] + -0.498535f * c[2]);
                    *aovs++ = -0.969256f * c[0] + (1.875991f * c[1] + 0.041556f * c[2]);
                    *aovs++ = 0.055648f * c[0] + (-0.204043f * c[1] + 1.057311f * c[2]);
                    *aovs++ = 1.f;
                    result = spec;
                } break;
            }
        }
    }
    result = result * ray_weight;
    spectrum_to_xyz(sc, result, wl, xyz);
}

// a1/a2  SamplingIntegrator::render + render_block (integrator.cpp:31-101)
static void render(const Scene &sc, const msk_render_params &prm, float *film, Counters *total, int n_threads,
                   const AovSpec *aov = nullptr, const msk_direct_params *direct = nullptr) {
    const int n_ch = 5 + (aov ? aov->channels : 0);
    const int W = sc.film.width, H = sc.film.height;
    // film.cpp:12-21: the crop window; the block schedule and the sensor stay those of the full film (integrator.cpp:45)
    const bool whole = sc.film.crop_size[0] == 0 && sc.film.crop_size[1] == 0;
    const int CX = whole ? 0 : sc.film.crop_offset[0], CY = whole ? 0 : sc.film.crop_offset[1];
    const int CW = whole ? W : sc.film.crop_size[0], CH = whole ? H : sc.film.crop_size[1];
    const int border = (int) std::ceil(sc.film.filter_radius - .5f);      // rfilter.cpp:22
    std::vector<BlockDesc> blocks = spiral_blocks(W, H, prm.block_size);
    std::vector<ImageBlock> done(blocks.size());
    std::atomic<size_t> next{0};
    std::mutex mtx;
    const uint32_t bstride = prm.block_stride ? prm.block_stride : 1, sstride = prm.sample_stride ? prm.sample_stride : 1;
    auto worker = [&]() {
        Counters cnt;
        for (;;) {
            size_t id = next.fetch_add(1);
            if (id >= blocks.size()) break;
            if (id % bstride != prm.block_first) continue;
            const BlockDesc &bd = blocks[id];
            // The reference renders every block of the full film and lets accumulate_2d clip it against the storage
            // (imageblock.cpp:133-150); a block whose bordered area misses the crop window is clipped to nothing there, so it is
            // skipped here (and by the GPU side, msk_gpu.h: msk_film_desc) instead of being rendered and thrown away.
            if (bd.off_x - border >= CX + CW || bd.off_x + bd.size_x + border <= CX || bd.off_y - border >= CY + CH || bd.off_y + bd.size_y + border <= CY) continue;
            ImageBlock blk;
            blk.off_x = bd.off_x; blk.off_y = bd.off_y; blk.channels = n_ch;
            blk.warn_negative = aov == nullptr;                    // integrator.cpp:59-60: !has_aovs
            blk.init(bd.size_x, bd.size_y, &sc.film, true);
            std::vector<float> v((size_t) n_ch);
            Sampler sampler; sampler.mode = prm.rng_mode;
            if (prm.rng_mode == MSK_RNG_PCG_BLOCK)                // D2; independent.cpp:20-26
                sampler.rng.seed(0x853c49e6748fea9bULL + prm.seed, 0xda3e39cb94b95bdbULL);
            for (int y = 0; y < bd.size_y; ++y)
                for (int x = 0; x < bd.size_x; ++x) {
                    V2 pos{(float) x + (float) bd.off_x, (float) y + (float) bd.off_y};
                    for (uint32_t s = 0; s < prm.spp; ++s) {
                        if (s < prm.sample_first || (s - prm.sample_first) % sstride != 0) continue;   // msk_gpu.h: s = first + k stride
                        if (prm.rng_mode == MSK_RNG_COUNTER)
                            sampler.key = counter_key(prm.seed, (uint32_t) ((y + bd.off_y) * W + (x + bd.off_x)), s);
                        V2 ps;
                        render_sample(sc, sampler, pos, prm, cnt, &ps, v.data(), aov, v.data() + 5, direct);
                        v[3] = 1.f; v[4] = 1.f;                    // integrator.cpp:119-123
                        blk.put(ps, v.data());
                    }
                }
            cnt.invalid += blk.invalid;
            done[id] = std::move(blk);
        }
        std::lock_guard<std::mutex> g(mtx);
        total->samples += cnt.samples; total->segments += cnt.segments; total->shadow_rays += cnt.shadow_rays; total->invalid += cnt.invalid;
        tallies_flush();
    };
    std::vector<std::thread> pool;
    for (int i = 0; i < std::max(1, n_threads); ++i) pool.emplace_back(worker);
    for (auto &t : pool) t.join();
    std::fill(film, film + (size_t) CW * CH * n_ch, 0.f);          // hdrfilm.cpp:37-39
    for (size_t id = 0; id < blocks.size(); ++id)                  // D6
        if (!done[id].data.empty()) film_put(film, CW, CH, done[id], CX, CY);
}

}  // namespace orc

// ===========================================================================
// C entry points (ctypes)
// ===========================================================================
// the rays of a batch are independent: split them over the host's threads (brute force over a 146 k-triangle scene is
// 3 ms per ray on one core)
template <typename F> static void for_rays(uint64_t n, F body) {
    unsigned nt = std::thread::hardware_concurrency();
    if (const char *e = getenv("MSK_ORACLE_THREADS")) nt = (unsigned) atoi(e);
    nt = std::max(1u, std::min(nt, 64u));
    if (n < 4096 || nt == 1) { for (uint64_t i = 0; i < n; ++i) body(i); orc::tallies_flush(); return; }
    std::vector<std::thread> pool;
    std::atomic<uint64_t> next{0};
    for (unsigned t = 0; t < nt; ++t)
        pool.emplace_back([&]() { for (;;) { const uint64_t b = next.fetch_add(256); if (b >= n) break; for (uint64_t i = b; i < std::min(n, b + 256); ++i) body(i); } orc::tallies_flush(); });
    for (auto &t : pool) t.join();
}
using namespace orc;
extern "C" {

// the ABI's own structs; NULL for what the library refuses at scene creation (scene_extensions)
void *msk_oracle_scene_create_masks(const msk_scene_desc *d, const msk_scene_masks *em) { return scene_from_desc(d, em); }
void *msk_oracle_scene_create(const msk_scene_desc *d) { return msk_oracle_scene_create_masks(d, nullptr); }
// everything msk_scene_lens holds; the entry points above and below are this one with lens = NULL
void *msk_oracle_scene_create_lens(const msk_scene_desc *d, const msk_scene_lens *el) {
    return el ? scene_from_desc(d, &el->lights.masks, el->lights.n_lights, el->lights.lights, el->lens) : scene_from_desc(d, nullptr);
}
void *msk_oracle_scene_create_lights(const msk_scene_desc *d, const msk_scene_lights *el) {
    return el ? scene_from_desc(d, &el->masks, el->n_lights, el->lights) : scene_from_desc(d, nullptr);
}
// reads and clears the path tallies (see PathTally): out receives msk_oracle_path_tally_count() values
// (these two keep answering for the fifteen tallies they always had, so that a caller written for them reads what it expects)
int msk_oracle_path_tally_count() { return (int) kTallyPlasticCoat; }
void msk_oracle_path_tallies(uint64_t *out) { path_flush(); for (int i = 0; i < kTallyPlasticCoat; ++i) out[i] = g_path[i].exchange(0); }
// ... and these two for twenty-five, the plastics' ten behind the fifteen.  The name is historical: they were all there were when the
// pair was introduced, and a binding written then asserts the count; msk_oracle_path_tally_total / _tallies_first below read all of them
int msk_oracle_path_tally_count_all() { return kTallyCountPlastics; }
void msk_oracle_path_tallies_all(uint64_t *out) { path_flush(); for (int i = 0; i < kTallyCountPlastics; ++i) out[i] = g_path[i].exchange(0); }
// ... and these two for every tally there is, however many are appended later: the caller says how many it knows (n <= total) and
// reads and clears those; what it does not know stays untouched.  The two pairs above are this with n = 15 and n = 25, and keep
// those answers so that a caller written for them reads what it expects.
int msk_oracle_path_tally_total() { return (int) kTallyCount; }
int msk_oracle_path_tallies_first(uint64_t *out, int n) {
    if (n < 0 || n > (int) kTallyCount) return -1;
    path_flush();
    for (int i = 0; i < n; ++i) out[i] = g_path[i].exchange(0);
    return 0;
}

// ---- known-answer hooks of the features restated from include/msk_gpu.h (shaped like msk_oracle_bsdf_sample2) ----
static S4 load4(const float *p) { S4 r; for (int i = 0; i < 4; ++i) r.v[i] = p[i]; return r; }
static void store4(float *p, S4 v) { for (int i = 0; i < 4; ++i) p[i] = v.v[i]; }
// texture `texture` (1-based) of the scene at uv, four wavelengths: what a diffuse BSDF's reflectance is there (scale 1)
void msk_oracle_eval_texture(void *s, uint32_t texture, const float *uv2, const float *wl4, float *out4) {
    const Scene &sc = *(Scene *) s;
    msk_bsdf_desc b{}; b.reflectance_texture = texture; b.reflectance_scale = 1.f;
    store4(out4, reflectance_eval(sc, reflectance_at(sc, b, V2{uv2[0], uv2[1]}), load4(wl4)));
}
int msk_oracle_env_eval(void *s, const float *dir3, const float *wl4, float *out_radiance4, float *out_pdf) {
    const Scene &sc = *(Scene *) s;
    if (!sc.env_is_image) return -1;
    float sin_theta;
    const V2 uv = env_dir_to_uv(sc.envmap, mk3(dir3[0], dir3[1], dir3[2]), &sin_theta);
    store4(out_radiance4, env_radiance(sc, uv, load4(wl4)));
    *out_pdf = env_pdf(sc.envmap, uv, sin_theta);
    return 0;
}
int msk_oracle_env_sample(void *s, const float *u2, float *out_dir3, float *out_uv2, float *out_pdf) {
    const Scene &sc = *(Scene *) s;
    if (!sc.env_is_image) return -1;
    V2 uv;
    const V3 d = env_sample(sc.envmap, V2{u2[0], u2[1]}, &uv, out_pdf);
    out_dir3[0] = d.x; out_dir3[1] = d.y; out_dir3[2] = d.z; out_uv2[0] = uv.x; out_uv2[1] = uv.y;
    return 0;
}
// the next-event sample of point emitter `emitter` from p: out_d_dist4 = {d, dist}, out_value4 (without the light-selection factor)
int msk_oracle_point_sample(void *s, uint32_t emitter, const float *p3, const float *wl4, float *out_d_dist4, float *out_value4) {
    const Scene &sc = *(Scene *) s;
    if (emitter >= sc.emitters.size() || sc.emitters[emitter].type != MSK_EMITTER_POINT) return -1;
    V3 d; float dist, pdf;
    const S4 v = point_sample(sc.point_pos[emitter], mk3(p3[0], p3[1], p3[2]), emitter_radiance(sc, (int) emitter, load4(wl4)), &d, &dist, &pdf);
    out_d_dist4[0] = d.x; out_d_dist4[1] = d.y; out_d_dist4[2] = d.z; out_d_dist4[3] = dist;
    store4(out_value4, v);
    return 0;
}
// the next-event sample of the spot or directional emitter `emitter`, as msk_gpu_light_sample gives it: out_d_dist4 = {d, dist}, out_value4
// (the value zeros where f == 0, everything zeros where dist == 0)
int msk_oracle_light_sample(void *s, uint32_t emitter, const float *p3, const float *wl4, float *out_d_dist4, float *out_value4) {
    const Scene &sc = *(Scene *) s;
    if (emitter >= sc.emitters.size() || (sc.emitters[emitter].type != MSK_EMITTER_SPOT && sc.emitters[emitter].type != MSK_EMITTER_DIRECTIONAL)) return -1;
    Interaction ref; ref.p = mk3(p3[0], p3[1], p3[2]);
    S4 v;
    const DirectSample ds = emitter_sample_direct(sc, (int) emitter, ref, V2{0.f, 0.f}, load4(wl4), &v);
    out_d_dist4[0] = ds.d.x; out_d_dist4[1] = ds.d.y; out_d_dist4[2] = ds.d.z; out_d_dist4[3] = ds.dist;
    store4(out_value4, v);
    return 0;
}
// the delta lobe's value of conductor `bsdf` for cos_theta_i (zeros for cos_i <= 0)
int msk_oracle_conductor_sample(void *s, uint32_t bsdf, float cos_theta_i, const float *wl4, float *out_value4) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size() || sc.bsdfs[bsdf].type != MSK_BSDF_CONDUCTOR) return -1;
    BSDFSampleRec bs; bs.wo = mk3(0, 0, 0); bs.pdf = 0.f; bs.eta = 1.f; bs.sampled_type = 0;
    const float st = std::sqrt(std::max(0.f, 1.f - cos_theta_i * cos_theta_i));
    store4(out_value4, conductor_sample(sc, sc.bsdfs[bsdf], mk3(st, 0.f, cos_theta_i), load4(wl4), &bs));
    return 0;
}
// sample() / eval() of the decorated entry `bsdf` (an entry without a mask: opacity 1) as msk_gpu_mask_sample / _mask_eval give them:
// out_wo_pdf4 = {wo, pdf} (the null lobe: wo = -wi), out_flags4 = {eta, delta, null lobe, a direction was produced}
int msk_oracle_mask_sample(void *s, uint32_t bsdf, const float *uv2, const float *wi3, const float *sample1_u3, const float *wl4,
                           float *out_wo_pdf4, float *out_value4, float *out_flags4) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size()) return -1;
    const V2 uv{uv2[0], uv2[1]};
    const float a = mask_opacity(sc, (int) bsdf, uv);
    V3 wi = mk3(wi3[0], wi3[1], wi3[2]);
    V2 u{sample1_u3[1], sample1_u3[2]};
    const S4 wl = load4(wl4);
    BSDFSampleRec bs; S4 value;
    const bool null_lobe = !(u.x < a);
    if (null_lobe) {
        bs.wo = -wi; bs.pdf = 1.f - a; bs.eta = 1.f; bs.sampled_type = kNull; value = s4(1.f);
    } else {
        u.x = u.x / a;
        bool flipped; const msk_bsdf_desc *bb = bsdf_side(sc, sc.bsdfs[bsdf], &wi, &flipped);
        value = bsdf_sample(sc, *bb, reflectance_at(sc, *bb, uv), wi, sample1_u3[0], u, wl, &bs);
        if (flipped) bs.wo.z *= -1.f;
        bs.pdf = a * bs.pdf;
    }
    out_wo_pdf4[0] = bs.wo.x; out_wo_pdf4[1] = bs.wo.y; out_wo_pdf4[2] = bs.wo.z; out_wo_pdf4[3] = bs.pdf;
    store4(out_value4, value);
    out_flags4[0] = bs.eta; out_flags4[1] = (null_lobe || (bs.sampled_type & kDelta) != 0u || !bsdf_has_smooth_lobe(sc.bsdfs[bsdf])) ? 1.f : 0.f;
    out_flags4[2] = null_lobe ? 1.f : 0.f; out_flags4[3] = bs.sampled_type ? 1.f : 0.f;
    return 0;
}
int msk_oracle_mask_eval(void *s, uint32_t bsdf, const float *uv2, const float *wi3, const float *wo3, const float *wl4, float *out_a_pdf2, float *out_value4) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size()) return -1;
    const V2 uv{uv2[0], uv2[1]};
    const float a = mask_opacity(sc, (int) bsdf, uv);
    V3 wi = mk3(wi3[0], wi3[1], wi3[2]), wo = mk3(wo3[0], wo3[1], wo3[2]);
    bool flipped; const msk_bsdf_desc *bb = bsdf_side(sc, sc.bsdfs[bsdf], &wi, &flipped);
    if (flipped) wo.z *= -1.f;
    S4 v; float pdf;
    bsdf_eval_pdf(sc, *bb, reflectance_at(sc, *bb, uv), wi, wo, load4(wl4), &v, &pdf);
    out_a_pdf2[0] = a; out_a_pdf2[1] = a * pdf;
    store4(out_value4, v * a);
    return 0;
}
// The probes of a `plastic` / `roughplastic` entry, arguments and outputs as msk_gpu_plastic_sample / _plastic_eval /
// _roughplastic_sample / _roughplastic_eval take and give them (n points; the mask hooks' layout: a scene without a mask has opacity 1
// on every entry).  Non-zero for an entry out of range or of another type.
static int plastic_probe_sample(void *s, int32_t type, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wl,
                                float *out_wo_pdf, float *out_value, float *out_flags) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size() || sc.bsdfs[bsdf].type != type) return MSK_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n; ++i)
        msk_oracle_mask_sample(s, bsdf, uv + 2 * i, wi + 3 * i, sample1_u + 3 * i, wl + 4 * i, out_wo_pdf + 4 * i, out_value + 4 * i, out_flags + 4 * i);
    return 0;
}
static int plastic_probe_eval(void *s, int32_t type, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wl,
                              float *out_a_pdf, float *out_value) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size() || sc.bsdfs[bsdf].type != type) return MSK_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < n; ++i) msk_oracle_mask_eval(s, bsdf, uv + 2 * i, wi + 3 * i, wo + 3 * i, wl + 4 * i, out_a_pdf + 2 * i, out_value + 4 * i);
    return 0;
}
int msk_oracle_plastic_sample(void *s, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                              float *out_wo_pdf, float *out_value, float *out_flags) {
    return plastic_probe_sample(s, MSK_BSDF_PLASTIC, bsdf, n, uv, wi, sample1_u, wavelengths, out_wo_pdf, out_value, out_flags);
}
int msk_oracle_plastic_eval(void *s, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths, float *out_a_pdf, float *out_value) {
    return plastic_probe_eval(s, MSK_BSDF_PLASTIC, bsdf, n, uv, wi, wo, wavelengths, out_a_pdf, out_value);
}
int msk_oracle_roughplastic_sample(void *s, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *sample1_u, const float *wavelengths,
                                   float *out_wo_pdf, float *out_value, float *out_flags) {
    return plastic_probe_sample(s, MSK_BSDF_ROUGHPLASTIC, bsdf, n, uv, wi, sample1_u, wavelengths, out_wo_pdf, out_value, out_flags);
}
int msk_oracle_roughplastic_eval(void *s, uint32_t bsdf, uint64_t n, const float *uv, const float *wi, const float *wo, const float *wavelengths, float *out_a_pdf, float *out_value) {
    return plastic_probe_eval(s, MSK_BSDF_ROUGHPLASTIC, bsdf, n, uv, wi, wo, wavelengths, out_a_pdf, out_value);
}
// out2 = {fdr_int, ssw} of a plastic entry of either type, as this file computed them (D20)
int msk_oracle_plastic_constants(void *s, uint32_t bsdf, float *out2) {
    const Scene &sc = *(Scene *) s;
    if (bsdf >= sc.bsdfs.size() || !is_plastic(sc.bsdfs[bsdf])) return MSK_ERR_INVALID_ARG;
    out2[0] = sc.plastic_k[bsdf].fdr_int; out2[1] = sc.plastic_k[bsdf].ssw;
    return 0;
}
void msk_oracle_scene_destroy(void *s) { delete (Scene *) s; }
void msk_oracle_set_bvh(void *s, int on) { ((Scene *) s)->use_bvh = on; }
void msk_oracle_set_libm(int on) { g_use_libm = on; }
void msk_oracle_set_trace(int on) { g_trace_path = on; }
// reads and clears the intersection tallies (see g_isect)
void msk_oracle_isect_counters(uint64_t *out8) { isect_flush(); for (int i = 0; i < 8; ++i) out8[i] = g_isect[i].exchange(0); }

int msk_oracle_render(void *s, const msk_render_params *prm, float *film, msk_stats *stats, int n_threads) {
    if (int rc = lens_refusal(*(Scene *) s, *prm)) return rc;
    Counters c;
    auto t0 = std::chrono::steady_clock::now();
    render(*(Scene *) s, *prm, film, &c, n_threads);
    auto t1 = std::chrono::steady_clock::now();
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->samples = c.samples; stats->segments = c.segments; stats->shadow_rays = c.shadow_rays; stats->invalid_samples = c.invalid;
        stats->ms_total = std::chrono::duration<float, std::milli>(t1 - t0).count();
    }
    return 0;
}

int msk_oracle_render_aov(void *s, const msk_render_params *prm, const int32_t *aov_types, uint32_t n_aovs, float *film,
                          msk_stats *stats, int n_threads) {
    AovSpec spec;
    for (uint32_t i = 0; i < n_aovs; ++i) {
        int w = AovSpec::width(aov_types[i]);
        if (w < 0) return -1;
        spec.types.push_back(aov_types[i]); spec.channels += w;
    }
    if (int rc = lens_refusal(*(Scene *) s, *prm)) return rc;
    Counters c;
    render(*(Scene *) s, *prm, film, &c, n_threads, &spec);
    if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->samples = c.samples; stats->segments = c.segments; stats->shadow_rays = c.shadow_rays; stats->invalid_samples = c.invalid; }
    return 0;
}

int msk_oracle_sample_pixels(void *s, const msk_render_params *prm, uint64_t n_pixels, const int32_t *pixels,
                             float *out_xyz, float *out_pos) {
    const Scene &sc = *(Scene *) s;
    if (prm->rng_mode != MSK_RNG_COUNTER) return MSK_ERR_UNSUPPORTED;      // counter RNG only, as msk_gpu_sample_pixels
    Counters cnt;
    for (uint64_t i = 0; i < n_pixels; ++i) {
        int x = pixels[2 * i], y = pixels[2 * i + 1];
        for (uint32_t sidx = 0; sidx < prm->spp; ++sidx) {
            Sampler sampler; sampler.mode = MSK_RNG_COUNTER;
            sampler.key = counter_key(prm->seed, (uint32_t) (y * sc.film.width + x), sidx);
            V2 ps; float xyz[3];
            render_sample(sc, sampler, V2{(float) x, (float) y}, *prm, cnt, &ps, xyz);
            size_t o = (size_t) i * prm->spp + sidx;
            out_xyz[o * 3 + 0] = xyz[0]; out_xyz[o * 3 + 1] = xyz[1]; out_xyz[o * 3 + 2] = xyz[2];
            if (out_pos) { out_pos[o * 2] = ps.x; out_pos[o * 2 + 1] = ps.y; }
        }
    }
    return 0;
}

// ---- the "direct" integrator (msk_gpu.h at msk_direct_params).  Non-zero where the library refuses: a scene that holds a mask,
// MSK_RNG_PCG_BLOCK, a count above 4096, both counts 0
int msk_oracle_render_direct(void *s, const msk_render_params *prm, const msk_direct_params *direct, float *film, msk_stats *stats, int n_threads) {
    const Scene &sc = *(Scene *) s;
    if (int rc = lens_refusal(sc, *prm)) return rc;
    if (int rc = direct_refusal(sc, *prm, *direct)) return rc;
    Counters c;
    auto t0 = std::chrono::steady_clock::now();
    render(sc, *prm, film, &c, n_threads, nullptr, direct);
    auto t1 = std::chrono::steady_clock::now();
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->samples = c.samples; stats->segments = c.segments; stats->shadow_rays = c.shadow_rays; stats->invalid_samples = c.invalid;
        stats->ms_total = std::chrono::duration<float, std::milli>(t1 - t0).count();
    }
    return 0;
}
// like msk_gpu_sample_pixels_direct it honours sample_first / sample_stride: per listed pixel the owned samples, in order
int msk_oracle_sample_pixels_direct(void *s, const msk_render_params *prm, const msk_direct_params *direct, uint64_t n_pixels, const int32_t *pixels,
                                    float *out_xyz, float *out_pos) {
    const Scene &sc = *(Scene *) s;
    if (int rc = lens_refusal(sc, *prm)) return rc;
    if (int rc = direct_refusal(sc, *prm, *direct)) return rc;
    const uint32_t stride = prm->sample_stride ? prm->sample_stride : 1;
    Counters cnt;
    size_t o = 0;
    for (uint64_t i = 0; i < n_pixels; ++i) {
        const int x = pixels[2 * i], y = pixels[2 * i + 1];
        for (uint64_t sidx = prm->sample_first; sidx < prm->spp; sidx += stride, ++o) {
            Sampler sampler; sampler.mode = MSK_RNG_COUNTER;
            sampler.key = counter_key(prm->seed, (uint32_t) (y * sc.film.width + x), (uint32_t) sidx);
            V2 ps; float xyz[3];
            render_sample(sc, sampler, V2{(float) x, (float) y}, *prm, cnt, &ps, xyz, nullptr, nullptr, direct);
            out_xyz[o * 3 + 0] = xyz[0]; out_xyz[o * 3 + 1] = xyz[1]; out_xyz[o * 3 + 2] = xyz[2];
            if (out_pos) { out_pos[o * 2] = ps.x; out_pos[o * 2 + 1] = ps.y; }
        }
    }
    tallies_flush();
    return 0;
}
// Every factor of camera sample `sample` of pixel (px, py), before the weights and the counts are applied:
//   out_head 16 floats: the four wavelengths, the ray weight, the emission term, the spectral result (before the ray weight and spectrum_to_xyz)
//   out_counts 4 ints: primary hit (1 / 0), light samples drawn, BSDF samples drawn, pairs drawn in all
//   out_light_i  N x 5: {pair, emitter, point, shadow ray traced, occluded};  out_light_f  N x 6: {p_l, p_b, emitter_val * bsdf_val at 4 wavelengths}
//   out_bsdf_i   M x 5: {pair of the lobe choice, pair of the direction, traced, reached an emitter or environment, left the scene};  out_bsdf_f  M x 6: {p_b, p_e, bsdf_val * value at 4}
//   out_draws 3 + N + 2 M ints: every pair index the sample drew from, in order
int msk_oracle_direct_terms(void *s, const msk_render_params *prm, const msk_direct_params *direct, int32_t px, int32_t py, uint32_t sample,
                            float *out_head, int32_t *out_counts, int32_t *out_light_i, float *out_light_f, int32_t *out_bsdf_i, float *out_bsdf_f,
                            int32_t *out_draws) {
    const Scene &sc = *(Scene *) s;
    if (int rc = lens_refusal(sc, *prm)) return rc;
    if (int rc = direct_refusal(sc, *prm, *direct)) return rc;
    std::vector<uint32_t> log;
    Sampler sampler; sampler.mode = MSK_RNG_COUNTER; sampler.log = &log;
    sampler.key = counter_key(prm->seed, (uint32_t) (py * sc.film.width + px), sample);
    Counters cnt;
    DirectTerms t;
    V2 ps; float xyz[3];
    S4 wl, weight, spectral;
    render_sample(sc, sampler, V2{(float) px, (float) py}, *prm, cnt, &ps, xyz, nullptr, nullptr, direct, &t, &wl, &weight, &spectral);
    store4(out_head, wl); store4(out_head + 4, weight); store4(out_head + 8, t.emission); store4(out_head + 12, spectral);
    out_counts[0] = t.hit ? 1 : 0; out_counts[1] = (int32_t) t.light.size(); out_counts[2] = (int32_t) t.bsdf.size(); out_counts[3] = (int32_t) log.size();
    for (size_t i = 0; i < t.light.size(); ++i) {
        const DirectLightTerm &l = t.light[i];
        int32_t *oi = out_light_i + 5 * i; float *of = out_light_f + 6 * i;
        oi[0] = (int32_t) l.pair; oi[1] = l.emitter; oi[2] = l.point; oi[3] = l.shadow; oi[4] = l.occluded;
        of[0] = l.p_l; of[1] = l.p_b; store4(of + 2, l.prod);
    }
    for (size_t j = 0; j < t.bsdf.size(); ++j) {
        const DirectBsdfTerm &b = t.bsdf[j];
        int32_t *oi = out_bsdf_i + 5 * j; float *of = out_bsdf_f + 6 * j;
        oi[0] = (int32_t) b.pair_lobe; oi[1] = (int32_t) b.pair_dir; oi[2] = b.traced; oi[3] = b.reached; oi[4] = b.escaped;
        of[0] = b.p_b; of[1] = b.p_e; store4(of + 2, b.prod);
    }
    for (size_t k = 0; k < log.size(); ++k) out_draws[k] = (int32_t) log[k];
    tallies_flush();
    return 0;
}
// reads and clears the direct tallies (see DirectTally): out receives msk_oracle_direct_tally_count() values
// (these two keep answering for their twenty-one)
int msk_oracle_direct_tally_count() { return kDirTallyCountFirst; }
void msk_oracle_direct_tallies(uint64_t *out) { direct_flush(); for (int i = 0; i < kDirTallyCountFirst; ++i) out[i] = g_direct[i].exchange(0); }
// ... and these two for all of them, the delta lights' seven behind the twenty-one
int msk_oracle_direct_tally_count_all() { return (int) kDirTallyCount; }
void msk_oracle_direct_tallies_all(uint64_t *out) { direct_flush(); for (int i = 0; i < kDirTallyCount; ++i) out[i] = g_direct[i].exchange(0); }

int msk_oracle_trace_closest(void *s, uint64_t n, const float *rays, float *out_hit) {
    const Scene &sc = *(Scene *) s;
    for_rays(n, [&](uint64_t i) {
        const float *r = rays + i * 8;
        Ray ray{mk3(r[0], r[1], r[2]), mk3(r[4], r[5], r[6]), r[3], r[7]};
        Hit h = closest_hit(sc, ray);
        float *o = out_hit + i * 4;
        o[0] = h.valid ? h.t : kInf; o[1] = h.valid ? h.u : 0.f; o[2] = h.valid ? h.v : 0.f;
        uint32_t p = h.valid ? h.prim : 0xffffffffu; std::memcpy(&o[3], &p, 4);
    });
    return 0;
}
int msk_oracle_trace_any(void *s, uint64_t n, const float *rays, uint8_t *out) {
    const Scene &sc = *(Scene *) s;
    for_rays(n, [&](uint64_t i) {
        const float *r = rays + i * 8;
        Ray ray{mk3(r[0], r[1], r[2]), mk3(r[4], r[5], r[6]), r[3], r[7]};
        out[i] = any_hit(sc, ray) ? 1 : 0;
    });
    return 0;
}

// ---- known-answer hooks ----------------------------------------------------
void msk_oracle_pcg32(uint64_t initstate, uint64_t initseq, int n, uint32_t *out_u32, float *out_f32,
                      uint64_t *out_state_inc) {
    PCG32 a; a.seed(initstate, initseq);
    if (out_state_inc) { out_state_inc[0] = a.state; out_state_inc[1] = a.inc; }
    PCG32 b = a;
    for (int i = 0; i < n; ++i) { if (out_u32) out_u32[i] = a.next_uint32(); if (out_f32) out_f32[i] = b.next_float32(); }
}
void msk_oracle_counter_pair(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t pair, float *out2) {
    counter_pair(counter_key(seed, pixel, sample), pair, &out2[0], &out2[1]);
}
void msk_oracle_constants(float *out3) { out3[0] = kEpsilon; out3[1] = kRayEpsilon; out3[2] = kShadowEpsilon; }
void msk_oracle_sample_wavelength(float u, float *wl4, float *w4) {
    S4 a, b; sample_wavelength(u, &a, &b);
    for (int i = 0; i < 4; ++i) { wl4[i] = a.v[i]; w4[i] = b.v[i]; }
}
static const Scene kNoScene{};    // the BSDF KAT entry points below take bare descs: none of them names a tabulated spectrum
// KAT hook: RegularSpectrum::eval (regular.cpp:73-91,148) of a table at four wavelengths
void msk_oracle_regular_eval(float lambda_min, float lambda_max, const float *values, uint32_t size, const float *wl4, float *out4) {
    Scene::RegularTable t;
    t.range_x = lambda_min;
    t.inv_interval = (float) (1.0 / (((double) lambda_max - (double) lambda_min) / (double) (size - 1)));
    t.pdf.assign(values, values + size);
    S4 w; for (int i = 0; i < 4; ++i) w.v[i] = wl4[i];
    S4 r = regular_eval(t, w);
    for (int i = 0; i < 4; ++i) out4[i] = r.v[i];
}
// KAT hook: 0 / 1 = the checkerboard shows color0 / color1 at uv
int msk_oracle_checkerboard(const msk_texture_desc *t, float u, float v) { return checkerboard_lookup(*t, V2{u, v}) == t->color0 ? 0 : 1; }
void msk_oracle_srgb_model_eval(const float *coeff3, const float *wl4, float *out4) {
    S4 w; for (int i = 0; i < 4; ++i) w.v[i] = wl4[i];
    S4 r = srgb_model_eval(coeff3, w);
    for (int i = 0; i < 4; ++i) out4[i] = r.v[i];
}
void msk_oracle_coordinate_system(const float *n3, float *s3, float *t3) {
    V3 s, t; coordinate_system(mk3(n3[0], n3[1], n3[2]), &s, &t);
    s3[0] = s.x; s3[1] = s.y; s3[2] = s.z; t3[0] = t.x; t3[1] = t.y; t3[2] = t.z;
}
void msk_oracle_warps(const float *u2, float *tri2, float *disk2, float *hemi3) {
    V2 u{u2[0], u2[1]};
    V2 a = square_to_uniform_triangle(u), b = square_to_uniform_disk_concentric(u);
    V3 c = square_to_cosine_hemisphere(u);
    tri2[0] = a.x; tri2[1] = a.y; disk2[0] = b.x; disk2[1] = b.y; hemi3[0] = c.x; hemi3[1] = c.y; hemi3[2] = c.z;
}
void msk_oracle_det_math(float x, float *out4) {   // sin, cos, atanh, cosh
    det_sincos(x, &out4[0], &out4[1]); out4[2] = det_atanh(x); out4[3] = det_cosh(x);
}
void msk_oracle_det_math2(float x, float *out2) { out2[0] = det_atan(x); out2[1] = det_tan(x); }
// BSDF layer hooks: wi/wo in the local shading frame, twosided handled like the integrator does
void msk_oracle_bsdf_eval(const msk_bsdf_desc *bsdfs, int n, int id, const float *wi3, const float *wo3, const float *wl4,
                          float *val4, float *pdf) {
    Scene sc; sc.bsdfs.assign(bsdfs, bsdfs + n);
    V3 wi = mk3(wi3[0], wi3[1], wi3[2]), wo = mk3(wo3[0], wo3[1], wo3[2]);
    S4 wl; for (int i = 0; i < 4; ++i) wl.v[i] = wl4[i];
    bool flipped; const msk_bsdf_desc *b = bsdf_side(sc, sc.bsdfs[id], &wi, &flipped);
    if (flipped) wo.z *= -1.f;
    S4 v; bsdf_eval_pdf(kNoScene, *b, Reflectance{b->reflectance, b->reflectance_scale, 0u}, wi, wo, wl, &v, pdf);
    for (int i = 0; i < 4; ++i) val4[i] = v.v[i];
}
void msk_oracle_bsdf_sample(const msk_bsdf_desc *bsdfs, int n, int id, const float *wi3, const float *u2, const float *wl4,
                            float *wo3, float *pdf, float *weight4) {
    Scene sc; sc.bsdfs.assign(bsdfs, bsdfs + n);
    V3 wi = mk3(wi3[0], wi3[1], wi3[2]);
    S4 wl; for (int i = 0; i < 4; ++i) wl.v[i] = wl4[i];
    bool flipped; const msk_bsdf_desc *b = bsdf_side(sc, sc.bsdfs[id], &wi, &flipped);
    BSDFSampleRec bs; S4 w = bsdf_sample(kNoScene, *b, Reflectance{b->reflectance, b->reflectance_scale, 0u}, wi, 0.f, V2{u2[0], u2[1]}, wl, &bs);
    if (flipped) bs.wo.z *= -1.f;
    wo3[0] = bs.wo.x; wo3[1] = bs.wo.y; wo3[2] = bs.wo.z; *pdf = bs.pdf;
    for (int i = 0; i < 4; ++i) weight4[i] = w.v[i];
}
// as above with the lobe-selection sample, returning BSDFSample::eta and sampled_type too
void msk_oracle_bsdf_sample2(const msk_bsdf_desc *bsdfs, int n, int id, const float *wi3, float sample1, const float *u2,
                             const float *wl4, float *wo3, float *pdf, float *weight4, float *eta, uint32_t *sampled_type) {
    Scene sc; sc.bsdfs.assign(bsdfs, bsdfs + n);
    V3 wi = mk3(wi3[0], wi3[1], wi3[2]);
    S4 wl; for (int i = 0; i < 4; ++i) wl.v[i] = wl4[i];
    bool flipped; const msk_bsdf_desc *b = bsdf_side(sc, sc.bsdfs[id], &wi, &flipped);
    BSDFSampleRec bs; S4 w = bsdf_sample(kNoScene, *b, Reflectance{b->reflectance, b->reflectance_scale, 0u}, wi, sample1, V2{u2[0], u2[1]}, wl, &bs);
    if (flipped) bs.wo.z *= -1.f;
    wo3[0] = bs.wo.x; wo3[1] = bs.wo.y; wo3[2] = bs.wo.z; *pdf = bs.pdf; *eta = bs.eta; *sampled_type = bs.sampled_type;
    for (int i = 0; i < 4; ++i) weight4[i] = w.v[i];
}
// filters/gaussian.cpp:10-20 + rfilter.cpp:12-27 (host side of the reference; libm expf)
void msk_oracle_gaussian_filter(float stddev, float *radius, float *lut33, float *scale_factor, int *border) {
    float r = 4 * stddev, alpha = -1.f / (2.f * stddev * stddev), bias = std::exp(alpha * r * r);
    float sum = 0.f;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) {
        float x = float(r * i) / MSK_FILTER_RESOLUTION;
        lut33[i] = std::max(0.f, std::exp(alpha * x * x) - bias);
        sum += lut33[i];
    }
    lut33[MSK_FILTER_RESOLUTION] = 0;
    *scale_factor = float(MSK_FILTER_RESOLUTION) / r;
    *border = (int) std::ceil(r - .5f);
    sum *= 2 * r / MSK_FILTER_RESOLUTION;
    float normalization = 1.0f / sum;
    for (int i = 0; i < MSK_FILTER_RESOLUTION; ++i) lut33[i] *= normalization;
    *radius = r;
}
// sensors/perspective.cpp:11-19 + core/transform.h:169-187 (host side; evaluated in
// fp64 and rounded once — Eigen's fp32 4x4 inverse is not reproducible without Eigen)
void msk_oracle_perspective_camera(float fov, float near_, float far_, int width, int height,
                                   const float *origin3, const float *target3, const float *up3,
                                   float *sample_to_camera16, float *to_world16) {
    double aspect = width / (double) height;
    double recip = 1.0 / ((double) far_ - (double) near_);
    double cot = 1.0 / std::tan(((double) (fov / 2.0f)) * (3.14159265358979323846 / 180.0));
    // camera_to_sample = S(w,h,1) * S(-.5,-.5*aspect,1) * T(-1,-1/aspect,0) * P
    // sample_to_camera = P^-1 * T^-1 * S2^-1 * S1^-1 applied to (px,py,0,1)
    // P = [cot 0 0 0; 0 cot 0 0; 0 0 far*recip -near*far*recip; 0 0 1 0]
    // P^-1 = [1/cot 0 0 0; 0 1/cot 0 0; 0 0 0 1; 0 0 -1/(near*far*recip) 1/near]
    double A = far_ * recip, B = -(double) near_ * far_ * recip;
    double Pinv[16] = {1 / cot, 0, 0, 0, 0, 1 / cot, 0, 0, 0, 0, 0, 1, 0, 0, 1 / B, -A / B};
    double sx = 1.0 / width / -0.5, sy = 1.0 / height / (-0.5 * aspect);
    // M = T^-1 * S2^-1 * S1^-1 : x' = sx*x + 1, y' = sy*y + 1/aspect, z' = z
    double M[16] = {sx, 0, 0, 1, 0, sy, 0, 1 / aspect, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0;
            for (int k = 0; k < 4; ++k) acc += Pinv[i * 4 + k] * M[k * 4 + j];
            sample_to_camera16[i * 4 + j] = (float) acc;
        }
    // lookat (transform.h:169-178)
    auto nrm = [](double *v) { double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= l; v[1] /= l; v[2] /= l; };
    auto crs = [](const double *a, const double *b, double *c) {
        c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; };
    double dir[3] = {(double) target3[0] - origin3[0], (double) target3[1] - origin3[1], (double) target3[2] - origin3[2]};
    nrm(dir);
    double up[3] = {up3[0], up3[1], up3[2]}; nrm(up);
    double left[3]; crs(up, dir, left); nrm(left);
    double nup[3]; crs(dir, left, nup); nrm(nup);
    for (int r = 0; r < 3; ++r) {
        to_world16[r * 4 + 0] = (float) left[r]; to_world16[r * 4 + 1] = (float) nup[r];
        to_world16[r * 4 + 2] = (float) dir[r]; to_world16[r * 4 + 3] = origin3[r];
    }
    to_world16[12] = 0; to_world16[13] = 0; to_world16[14] = 0; to_world16[15] = 1;
}
// (a scene with a lens: the ray through the lens' centre, u = (0.5, 0.5); msk_oracle_camera_sample takes the aperture sample)
void msk_oracle_camera_ray(void *s, float wavelength_sample, float px, float py, float *out_ray8, float *wl4, float *w4) {
    S4 a, b; Ray r = camera_ray(*(Scene *) s, wavelength_sample, V2{px, py}, &a, &b);
    out_ray8[0] = r.o.x; out_ray8[1] = r.o.y; out_ray8[2] = r.o.z; out_ray8[3] = r.mint;
    out_ray8[4] = r.d.x; out_ray8[5] = r.d.y; out_ray8[6] = r.d.z; out_ray8[7] = r.maxt;
    for (int i = 0; i < 4; ++i) { wl4[i] = a.v[i]; w4[i] = b.v[i]; }
}
// the camera ray of n film positions, shaped like msk_gpu_camera_sample: film_pos n * 2, aperture_u n * 2 (read only by a scene with a
// lens, may be NULL otherwise), out n * 8 = {o, tnear} {d, tfar}.  No tally moves.
int msk_oracle_camera_sample(void *s, uint64_t n, const float *film_pos2, const float *aperture_u2, float *out8) {
    const Scene &sc = *(Scene *) s;
    if (sc.has_lens && !aperture_u2) return -1;
    for (uint64_t i = 0; i < n; ++i) {
        S4 a, b;
        const V2 u = sc.has_lens ? V2{aperture_u2[2 * i], aperture_u2[2 * i + 1]} : V2{0.5f, 0.5f};
        const Ray r = camera_ray(sc, 0.5f, V2{film_pos2[2 * i], film_pos2[2 * i + 1]}, &a, &b, u, false);
        float *o = out8 + 8 * i;
        o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z; o[3] = r.mint; o[4] = r.d.x; o[5] = r.d.y; o[6] = r.d.z; o[7] = r.maxt;
    }
    return 0;
}
int msk_oracle_spiral_blocks(int w, int h, int block_size, int max_out, int32_t *out4) {
    auto b = spiral_blocks(w, h, block_size);
    for (size_t i = 0; i < b.size() && (int) i < max_out; ++i) {
        out4[i * 4] = b[i].off_x; out4[i * 4 + 1] = b[i].off_y; out4[i * 4 + 2] = b[i].size_x; out4[i * 4 + 3] = b[i].size_y;
    }
    return (int) b.size();
}
// one ImageBlock::put into a fresh bordered block; returns the (size+2b)^2*5 buffer
void msk_oracle_block_put(const msk_film_desc *film, int off_x, int off_y, int size_x, int size_y, int n,
                          const float *pos2, const float *val5, float *out) {
    ImageBlock b; b.off_x = off_x; b.off_y = off_y; b.init(size_x, size_y, film, true);
    for (int i = 0; i < n; ++i) b.put(V2{pos2[2 * i], pos2[2 * i + 1]}, val5 + 5 * i);
    std::memcpy(out, b.data.data(), b.data.size() * sizeof(float));
}
// the same puts into a bordered block that already holds earlier ones (inout): one block's sample list fed in pieces
void msk_oracle_block_put_acc(const msk_film_desc *film, int off_x, int off_y, int size_x, int size_y, int n,
                              const float *pos2, const float *val5, float *inout) {
    ImageBlock b; b.off_x = off_x; b.off_y = off_y; b.init(size_x, size_y, film, true);
    std::memcpy(b.data.data(), inout, b.data.size() * sizeof(float));
    for (int i = 0; i < n; ++i) b.put(V2{pos2[2 * i], pos2[2 * i + 1]}, val5 + 5 * i);
    std::memcpy(inout, b.data.data(), b.data.size() * sizeof(float));
}
void msk_oracle_mesh_tables(void *s, uint32_t mesh, float *area, float *cdf, int max_cdf) {
    const Scene &sc = *(Scene *) s;
    *area = sc.mesh_area[mesh];
    for (size_t i = 0; i < sc.mesh_cdf[mesh].size() && (int) i < max_cdf; ++i) cdf[i] = sc.mesh_cdf[mesh][i];
}
// ext/rgb2spec/rgb2spec.c:56-119 rgb2spec_find_interval + rgb2spec_fetch, on a
// caller-supplied table (res, scale[res], data[3*res^3*3])
static int find_interval(const float *values, int size_, float x) {
    int left = 0, last_interval = size_ - 2, size = last_interval;
    while (size > 0) {
        int half = size >> 1, middle = left + half + 1;
        if (values[middle] <= x) { left = middle; size -= half + 1; } else { size = half; }
    }
    return std::min(left, last_interval);
}
void msk_oracle_rgb2spec_fetch(int res, const float *scale, const float *data, const float *rgb_, float *out) {
    int i = 0; float rgb[3];
    for (int j = 0; j < 3; ++j) rgb[j] = std::max(std::min(rgb_[j], 1.f), 0.f);
    for (int j = 1; j < 3; ++j) if (rgb[j] >= rgb[i]) i = j;
    float z = rgb[i], sc = (res - 1) / z, x = rgb[(i + 1) % 3] * sc, y = rgb[(i + 2) % 3] * sc;
    uint32_t xi = std::min((uint32_t) x, (uint32_t) (res - 2)), yi = std::min((uint32_t) y, (uint32_t) (res - 2)),
             zi = find_interval(scale, res, z), offset = (((i * res + zi) * res + yi) * res + xi) * 3, dx = 3,
             dy = 3 * res, dz = 3 * res * res;
    float x1 = x - xi, x0 = 1.f - x1, y1 = y - yi, y0 = 1.f - y1,
          z1 = (z - scale[zi]) / (scale[zi + 1] - scale[zi]), z0 = 1.f - z1;
    for (int j = 0; j < 3; ++j) {
        out[j] = ((data[offset] * x0 + data[offset + dx] * x1) * y0 +
                  (data[offset + dy] * x0 + data[offset + dy + dx] * x1) * y1) * z0 +
                 ((data[offset + dz] * x0 + data[offset + dz + dx] * x1) * y0 +
                  (data[offset + dz + dy] * x0 + data[offset + dz + dy + dx] * x1) * y1) * z1;
        offset++;
    }
}

}  // extern "C"
