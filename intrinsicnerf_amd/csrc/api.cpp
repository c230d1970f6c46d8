// api.cpp - whole-path entry point of the C ABI: enqueues the stage kernels for one ray batch.
// Replaces render_rays (object_level/run_nerf.py:415-528) / SSRTrainer.volumetric_rendering
// (SSR/training/trainer.py:717-808).  No host synchronisation, no allocation: all scratch lives in
// the caller's workspace.
#include <cstdint>
#include <cstdlib>

#include "draws.h"
#include "layout.h"

namespace {

constexpr int64_t kAlign = 256;
inline int64_t up(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

struct Plan {
    int64_t z_c, w_c, raw_c, z_s, z_f, raw_f, mlp_ws, mlp_ws_bytes, total;
    int ch_c, ch_f, s_f;
};

// which intermediate tensors the caller supplies as outputs (inerf_render_args): no workspace is reserved for those.
// raw is by far the largest (N x S x CH floats: ~6 GB for 32768 rays x 192 samples x 240 channels), and the SSR
// front-end asks for raw_coarse / raw_fine by default.
enum : unsigned { kHaveZc = 1, kHaveWc = 2, kHaveRawC = 4, kHaveZs = 8, kHaveZf = 16, kHaveRawF = 32 };

// Colour heads only on points with positive density (INERF_FLAG_GATE_COLOUR): a pass is gated when nobody outside the library sees its raw
// tensor and no noise is added to its sigma; which networks the flag does anything for is inerf_encode_mlp*'s business.  INERF_GATE=0: never.
// Wherever the gate is set, so is its one-product probe (INERF_FLAG_GATE_PROBE); INERF_PROBE=0: the gate without it.
constexpr uint32_t kGateFlags = INERF_FLAG_GATE_COLOUR | INERF_FLAG_GATE_PROBE;
uint32_t gate_flag(bool raw_provided, bool noise) {
    const char* e = std::getenv("INERF_GATE");
    if (raw_provided || noise || (e && e[0] == '0')) return 0u;
    const char* pr = std::getenv("INERF_PROBE");
    return INERF_FLAG_GATE_COLOUR | ((pr && pr[0] == '0') ? 0u : INERF_FLAG_GATE_PROBE);
}

unsigned provided(const inerf_render_args& a) {
    return (a.z_coarse ? kHaveZc : 0u) | (a.coarse.weights ? kHaveWc : 0u) | (a.raw_coarse ? kHaveRawC : 0u) |
           (a.z_samples ? kHaveZs : 0u) | (a.z_fine ? kHaveZf : 0u) | (a.raw_fine ? kHaveRawF : 0u);
}

Plan plan(const inerf_net_desc& net, int64_t n, int sc, int ni, uint32_t flags, unsigned have = 0) {
    Plan p{};
    p.ch_c = inerf_raw_channels(&net, flags, 0);
    p.ch_f = inerf_raw_channels(&net, flags, 1);
    p.s_f = sc + ni;
    int64_t off = 0;
    auto take = [&](int64_t floats, unsigned bit) {
        if (have & bit) return (int64_t)-1;
        int64_t o = off;
        off += up(floats * 4);
        return o;
    };
    p.z_c = take(n * sc, kHaveZc);
    p.w_c = ni > 0 ? take(n * sc, kHaveWc) : (int64_t)-1;   // the coarse weights are only needed for resampling
    p.raw_c = take(n * sc * p.ch_c, kHaveRawC);
    if (ni > 0) {
        p.z_s = take(n * ni, kHaveZs);
        p.z_f = take(n * p.s_f, kHaveZf);
        p.raw_f = take(n * p.s_f * p.ch_f, kHaveRawF);
    }
    // scratch of the encode+MLP launches (the SSR network's channel-split semantic head; the density gate's records - reserved whenever the
    // caller does not take the pass's raw tensor: whether noise keeps the gate off is only known at the call); one region serves both passes
    const uint32_t mlp_flags = flags & ~kGateFlags;
    const int64_t ws_c = inerf_encode_mlp_workspace_bytes(&net, n, sc, (mlp_flags & ~INERF_FLAG_ENDPOINT) | gate_flag(have & kHaveRawC, false));
    const int64_t ws_f = ni > 0 ? inerf_encode_mlp_workspace_bytes(&net, n, p.s_f, mlp_flags | gate_flag(have & kHaveRawF, false)) : 0;
    p.mlp_ws_bytes = ws_c > ws_f ? ws_c : ws_f;
    p.mlp_ws = off;
    off += up(p.mlp_ws_bytes);
    p.total = off;
    return p;
}

}  // namespace

extern "C" int64_t inerf_workspace_bytes(const inerf_net_desc* net, int64_t n_rays, int n_samples, int n_importance,
                                         uint32_t flags) {
    if (!net || !inerf::net_supported(*net) || n_rays < 0 || n_samples < 1 || n_importance < 0) return INERF_E_INVALID;
    return plan(*net, n_rays, n_samples, n_importance, flags).total;
}

extern "C" int64_t inerf_render_workspace_bytes(const inerf_render_args* a) {
    if (!a || !inerf::net_supported(a->net) || a->n_rays < 0 || a->n_samples < 1 || a->n_importance < 0) return INERF_E_INVALID;
    return plan(a->net, a->n_rays, a->n_samples, a->n_importance, a->flags, provided(*a)).total;
}

// The stage kernels' size limits for this pair of sample counts (include/inerf.h), so that a batch none of whose later stages can run
// is turned away before the first one is enqueued.
static bool sizes_supported(int sc, int ni) {
    static_assert(INERF_MAX_COARSE + INERF_MAX_IMPORTANCE <= INERF_MAX_SAMPLES, "the fine pass composites n_samples + n_importance");
    if (ni <= 0) return sc <= INERF_MAX_SAMPLES;                                      // inerf_composite alone
    return sc >= INERF_MIN_COARSE && sc <= INERF_MAX_COARSE && ni <= INERF_MAX_IMPORTANCE;   // inerf_sample_fine; the merged count then fits
}

// `d` null: the classic form.  Otherwise the drawn form: what the reference draws comes from the kernels (include/inerf.h, "Training draws").
static int render_impl(const inerf_render_args* a, const inerf_draw_args* d, void* stream) {
    const bool perturb = d && (d->flags & INERF_DRAW_PERTURB);
    const bool drawn_noise = d && d->noise_std > 0.0f;
    if (d) {
        if (!a) return INERF_E_INVALID;
        if (const int rc = inerf::draw_check(d, a->n_rays, INERF_DRAW_PERTURB)) return rc;
        if (a->t_rand || a->noise_coarse || a->noise_fine || (perturb && a->u)) return INERF_E_INVALID;
    }
    if (a && a->n_rays == 0)                                                          // empty batch: null pointers allowed
        return inerf::net_supported(a->net) && sizes_supported(a->n_samples, a->n_importance) ? INERF_OK : INERF_E_UNSUPPORTED;
    if (!a || !a->packed_coarse || !a->rays || !a->t_vals || a->n_rays < 0 || a->n_samples < 1 || a->n_importance < 0)
        return INERF_E_INVALID;
    if (!inerf::net_supported(a->net)) return INERF_E_UNSUPPORTED;
    if (a->n_importance > 0 && !a->u && !perturb) return INERF_E_INVALID;
    if (!sizes_supported(a->n_samples, a->n_importance)) return INERF_E_UNSUPPORTED;
    const Plan p = plan(a->net, a->n_rays, a->n_samples, a->n_importance, a->flags, provided(*a));
    if (p.total > 0 && (!a->workspace || a->workspace_bytes < p.total)) return INERF_E_WORKSPACE;
    char* ws = static_cast<char*>(a->workspace);
    auto f = [&](int64_t off) { return reinterpret_cast<float*>(ws + off); };
    const bool ssr = a->net.variant == INERF_VARIANT_SSR;
    const int n_cls = ssr ? a->net.n_classes : 0;
    const int64_t n = a->n_rays;
    const int sc = a->n_samples, ni = a->n_importance;
    int rc;

    // ---- coarse pass ----
    float* z_c = a->z_coarse ? a->z_coarse : f(p.z_c);
    inerf_draw_args dn{};                          // the stage calls' draw arguments: no flag but INERF_DRAW_FINE for the fine pass's noise
    if (d) {
        dn = *d;
        dn.flags = 0;
    }
    rc = perturb ? inerf_sample_coarse_drawn(a->rays, a->t_vals, nullptr, n, sc, a->flags, z_c, &dn, stream)
                 : inerf_sample_coarse(a->rays, a->t_vals, a->t_rand, n, sc, a->flags, z_c, stream);
    if (rc) return rc;
    float* raw_c = a->raw_coarse ? a->raw_coarse : f(p.raw_c);
    // the coarse net never emits the endpoint feature (trainer.py:751-755: endpoint_feat=False)
    const uint32_t mlp_flags = a->flags & ~kGateFlags;
    rc = inerf_encode_mlp_margin(&a->net, a->packed_coarse, a->rays, z_c, n, sc,
                                 (mlp_flags & ~INERF_FLAG_ENDPOINT) | gate_flag(a->raw_coarse != nullptr, a->noise_coarse != nullptr || drawn_noise), raw_c, a->status,
                                 a->status_rays, ws + p.mlp_ws, p.mlp_ws_bytes, nullptr, a->gate_state_coarse, stream);
    if (rc) return rc;
    inerf_composite_out oc = a->coarse;
    oc.feat = nullptr;
    if (ni > 0 && !oc.weights) oc.weights = f(p.w_c);
    rc = drawn_noise ? inerf_composite_drawn(raw_c, z_c, a->rays + 3, INERF_RAY_FLOATS, nullptr, n, sc, p.ch_c, oc.sem ? n_cls : 0, 0,
                                             a->flags, &oc, &dn, stream)
                     : inerf_composite(raw_c, z_c, a->rays + 3, INERF_RAY_FLOATS, a->noise_coarse, n, sc, p.ch_c, oc.sem ? n_cls : 0, 0,
                                       a->flags, &oc, stream);
    if (rc || ni == 0) return rc;

    // ---- resample, fine pass ----
    float* z_s = a->z_samples ? a->z_samples : f(p.z_s);
    float* z_f = a->z_fine ? a->z_fine : f(p.z_f);
    rc = perturb ? inerf_sample_fine_drawn(z_c, oc.weights, nullptr, n, sc, ni, a->flags, z_s, z_f, a->z_std, &dn, stream)
                 : inerf_sample_fine(z_c, oc.weights, a->u, n, sc, ni, a->flags, z_s, z_f, a->z_std, stream);
    if (rc) return rc;
    float* raw_f = a->raw_fine ? a->raw_fine : f(p.raw_f);
    const float* w_fine = a->packed_fine ? a->packed_fine : a->packed_coarse;   // run_nerf.py:506
    rc = inerf_encode_mlp_margin(&a->net, w_fine, a->rays, z_f, n, p.s_f, mlp_flags | gate_flag(a->raw_fine != nullptr, a->noise_fine != nullptr || drawn_noise), raw_f,
                                 a->status, a->status_rays, ws + p.mlp_ws, p.mlp_ws_bytes, nullptr, a->gate_state_fine, stream);
    if (rc) return rc;
    const bool ep = ssr && (a->flags & INERF_FLAG_ENDPOINT);
    inerf_composite_out of = a->fine;
    if (!ep) of.feat = nullptr;
    if (drawn_noise) {
        dn.flags = INERF_DRAW_FINE;
        return inerf_composite_drawn(raw_f, z_f, a->rays + 3, INERF_RAY_FLOATS, nullptr, n, p.s_f, p.ch_f, of.sem ? n_cls : 0,
                                     (ep && of.feat) ? INERF_ENDPOINT_DIM : 0, a->flags, &of, &dn, stream);
    }
    return inerf_composite(raw_f, z_f, a->rays + 3, INERF_RAY_FLOATS, a->noise_fine, n, p.s_f, p.ch_f, of.sem ? n_cls : 0,
                           (ep && of.feat) ? INERF_ENDPOINT_DIM : 0, a->flags, &of, stream);
}

extern "C" int inerf_render_rays(const inerf_render_args* a, void* stream) { return render_impl(a, nullptr, stream); }

extern "C" int inerf_render_rays_drawn(const inerf_render_args* a, const inerf_draw_args* draw, void* stream) {
    if (!draw) return INERF_E_INVALID;
    return render_impl(a, draw, stream);
}
