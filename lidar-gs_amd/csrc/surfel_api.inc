// surfel_api.inc -- extern "C" entry points of the surfel variant (included by surfel.hip).
// Counterpart of CudaRasterizer::Rasterizer::{forward,backward,visible_filter} of
// R2/cuda_rasterizer/rasterizer.h:31-114 / rasterizer_impl.cu:200-518.
#include "../../include/lidargs_rasterizer.h"
#include "../../include_surfel_pose/lidargs_surfel_pose.h"
#include <math.h>

namespace lg {

static_assert(SURFEL_BUFFERS.seg_planes == SF_SEG_PLANES, "lidargs_common.h SURFEL_BUFFERS carves the surfel blend's segment planes");
struct SfImgView { float* accum; uint32_t* n_contrib; uint2* ranges; float2* coltab; float2* rowtab; };
static size_t sf_img_carve(char* base, int W, int H, int tiles, SfImgView* v) {
    Carver c(base);
    SfImgView m;
    const size_t N = (size_t)W * H;
    m.accum = c.take<float>(3 * N); m.n_contrib = c.take<uint32_t>(2 * N); m.ranges = c.take<uint2>(tiles);
    m.coltab = c.take<float2>(W); m.rowtab = c.take<float2>(H);
    if (v) *v = m;
    return (size_t)(c.p - base) + 128;
}

// The surfels and the sensor as the preprocess and the per-surfel backward chain read them, and the backward's nine gradient rows: the
// entry points fill both BY FIELD NAME (as api.hip's SceneArgs / GradRows), so no helper below hangs on an argument's position.
namespace {
struct SfScene { int P = 0; const float* viewmatrix = nullptr; const float* means3D = nullptr; const float* scales = nullptr; const float* rotations = nullptr; const float* transMat_precomp = nullptr; const float* beams = nullptr; };
struct SfGradRows {   // dL_dnormal, dL_dtransMat, dL_dtransMat_2dtemp: optional
    float* dL_dmean2D = nullptr; float* dL_dnormal = nullptr; float* dL_dopacity = nullptr; float* dL_dcolor = nullptr; float* dL_dmean3D = nullptr;
    float* dL_dtransMat = nullptr; float* dL_dtransMat_2dtemp = nullptr; float* dL_dscale = nullptr; float* dL_drot = nullptr;
    bool required() const { return dL_dmean2D && dL_dopacity && dL_dcolor && dL_dmean3D && dL_dscale && dL_drot; }
    ZeroRows zero_rows() const {   // the rows the backward's first launch zeroes, with their widths (depth is written for every surfel by k_sf_gaussian_backward)
        ZeroRows zr; zr.add(dL_dmean2D, 4); zr.add(dL_dnormal, 3); zr.add(dL_dopacity, 1); zr.add(dL_dcolor, 2); zr.add(dL_dmean3D, 3); zr.add(dL_dtransMat, 9);
        zr.add(dL_dtransMat_2dtemp, 3); zr.add(dL_dscale, 2); zr.add(dL_drot, 4);
        return zr;
    }
};
}  // namespace
// the per-surfel chain's arguments; W, H, radii and depth (an output, not a gradient) are each caller's own
static SfGaussBwdArgs sf_gauss_bwd_args(const SfScene& sc, const SfGradRows& g, const float* gacc, const uint8_t* tlist, const uint16_t* tcount) {
    SfGaussBwdArgs ga;
    ga.P = sc.P; ga.view = sc.viewmatrix; ga.means3D = sc.means3D; ga.scales = sc.scales; ga.rotations = sc.rotations; ga.beams = sc.beams; ga.transMat = sc.transMat_precomp;
    ga.gacc = gacc; ga.tlist = tlist; ga.tcount = tcount; ga.dL_dmean2D = g.dL_dmean2D; ga.dL_dnormal = g.dL_dnormal; ga.dL_dopacity = g.dL_dopacity; ga.dL_dcolor = g.dL_dcolor;
    ga.dL_dmean3D = g.dL_dmean3D; ga.dL_dtransMat = g.dL_dtransMat; ga.dL_dtransMat_2dtemp = g.dL_dtransMat_2dtemp; ga.dL_dscale = g.dL_dscale; ga.dL_drot = g.dL_drot;
    return ga;
}
// The surfel preprocess' parameters of a whole width x height frame at tile height TH: everything but the arrays it writes.  The forward,
// the visible filter and the test hook (lidargs_debug_surfel_preprocess) all start from here, so the column step is the same value for each.
static SfPreArgs sf_pre_params(const SfScene& sc, const TileGrid& grid, float scale_modifier, float near_f, float far_f, int* radii, int* radii_xy) {
    SfPreArgs pa = SfPreArgs();
    pa.P = sc.P; pa.W = grid.W; pa.H = grid.H; pa.TH = grid.TH; pa.tiles_x = grid.tiles_x;
    pa.scale_modifier = scale_modifier; pa.near_f = near_f; pa.far_f = far_f;
    pa.col_step = 2 * 3.14159265358979323846f / (float)grid.W;
    pa.view = sc.viewmatrix; pa.means3D = sc.means3D; pa.scales = sc.scales; pa.rotations = sc.rotations; pa.beams = sc.beams;
    pa.radii = radii; pa.radii_xy = radii_xy;
    return pa;
}
// ... and what the full preprocess reads and writes on top (K2 has none of it)
static void sf_pre_outputs(SfPreArgs& pa, const float* opacities, const float* colors, const float* transMat, const GeomView& geom, int compact, int prune) {
    pa.opacities = opacities; pa.colors = colors; pa.transMat = transMat;
    pa.rec = geom.rec; pa.rowspan = geom.rowspan; pa.spans = geom.spans; pa.dkey = geom.key_a; pa.ids = geom.id_a;
    pa.inst_slots = reinterpret_cast<unsigned long long*>(geom.totals + LG_TOTALS_SLOT_WORD);
    pa.diag_slots = reinterpret_cast<unsigned long long*>(geom.totals + LG_TOTALS_DIAG_WORD);
    pa.key_span = geom.totals + LG_TOTALS_KEYSPAN_WORD;
    pa.compact = compact; pa.touched = geom.touched; pa.prune = prune;
}

}  // namespace lg

// The C parameter names the surfel entry points share onto the two structs, each stated once (bound by name, as api.hip's LG_*_ARGS).
#define SF_SCENE(sc, beams_)                                                                                                                                                                \
    lg::SfScene sc; sc.P = P; sc.viewmatrix = viewmatrix; sc.means3D = means3D; sc.scales = scales; sc.rotations = rotations; sc.transMat_precomp = transMat_precomp; sc.beams = beams_
#define SF_GRAD_ROWS(rows)                                                                                                                                                                  \
    lg::SfGradRows rows; rows.dL_dmean2D = dL_dmean2D; rows.dL_dnormal = dL_dnormal; rows.dL_dopacity = dL_dopacity; rows.dL_dcolor = dL_dcolor; rows.dL_dmean3D = dL_dmean3D;              \
    rows.dL_dtransMat = dL_dtransMat; rows.dL_dtransMat_2dtemp = dL_dtransMat_2dtemp; rows.dL_dscale = dL_dscale; rows.dL_drot = dL_drot
#define SF_CHECK(what) do { int rc_ = lg::api_check_launch(stream, debug, what); if (rc_) return rc_; } while (0)
#define SF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return lg::api_fail(LIDARGS_ERR_HIP, hipGetErrorString(e_)); } while (0)

extern "C" {

int lidargs_surfel_forward(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                           lidargs_alloc_fn image_alloc, void* image_user, int P, int D, int M, const float* background, int width,
                           int height, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                           const float* scales, float scale_modifier, const float* rotations, const float* transMat_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* cam_pos, const float* beam_inclinations,
                           int prefiltered, int lidar_far, int lidar_near, float* out_color, float* out_others, float* pixels, int* radii,
                           int* radii_xy, int debug, void* stream_) {
    (void)D; (void)M; (void)shs; (void)projmatrix; (void)cam_pos; (void)prefiltered; (void)pixels;   // `pixels` is never written by the reference either (R2/cr/forward.cu:522)
    hipStream_t stream = (hipStream_t)stream_;
    // (the surfel backward still adds with float atomics; the surfel variant returns its own median plane, others[5])
    if (const int rc = lg::refuse_modes("lidargs_surfel_forward")) return rc;
    if (P < 0 || width <= 0 || height < 2 || height > 65535) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel forward: bad sizes");
    if (colors_precomp == nullptr) return lg::api_fail(LIDARGS_ERR_NO_COLORS, "For non-RGB, provide precomputed Gaussian colors!");
    // transMat_precomp, as the reference treats it: its preprocess builds T from scales and rotations unconditionally (rect, normal,
    // sort depth, pixel centre: R2/cr/forward.cu:271-325) and its BLEND then reads the rows from transMat_precomp when that pointer is
    // there (R2/cr/rasterizer_impl.cu:332).  So both must be given; transMat_precomp alone is refused (the reference would read scales
    // from an empty tensor).
    if (transMat_precomp != nullptr && (!scales || !rotations))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel forward: transMat_precomp without scales and rotations (the reference's preprocess reads them even then, R2/cr/forward.cu:271-273)");
    if (!means3D || !opacities || !scales || !rotations || !viewmatrix || !beam_inclinations || !background || !out_color || !out_others || !radii || !radii_xy)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel forward: NULL required pointer");
    if (!geometry_alloc || !binning_alloc || !image_alloc) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel forward: NULL allocator");
    if (P == 0) return 0;
    const int TH = lg::tile_rows();
    const lg::TileGrid grid = lg::make_grid(width, height, TH);
    char* geom_p = geometry_alloc(geometry_user, lg::geom_carve(nullptr, (size_t)P, lg::SURFEL_BUFFERS, nullptr));
    char* img_p = image_alloc(image_user, lg::sf_img_carve(nullptr, width, height, grid.num_tiles(), nullptr));
    if (!geom_p || !img_p) return lg::api_fail(LIDARGS_ERR_ALLOC, "surfel forward: allocator returned NULL");
    lg::GeomView geom; lg::geom_carve(geom_p, (size_t)P, lg::SURFEL_BUFFERS, &geom);
    lg::SfImgView img; lg::sf_img_carve(img_p, width, height, grid.num_tiles(), &img);

    lg::prof_begin(stream, 0);
    lg::ImgView tabs = lg::ImgView(); tabs.coltab = img.coltab; tabs.rowtab = img.rowtab;
    lg::launch_setup_tables(beam_inclinations, width, height, tabs, stream);
    SF_SCENE(sc, beam_inclinations);
    lg::SfPreArgs pa = lg::sf_pre_params(sc, grid, scale_modifier, (float)lidar_near, (float)lidar_far, radii, radii_xy);
    lg::sf_pre_outputs(pa, opacities, colors_precomp, transMat_precomp, geom, lg::compact_spans(grid.tiles_x, height) ? 1 : 0,
                       lg::prune_footprints() ? 1 : 0);
    SF_HIP(hipMemsetAsync(geom.totals, 0, LG_TOTALS_WORDS * sizeof(uint32_t), stream));
    lg::launch_sf_preprocess(pa, false, stream);
    SF_CHECK("surfel preprocess");
    lg::prof_mark("preprocess", stream);

    // the binning as the 3-D variant's (api.hip bin_frame), at the fixed tile height
    const lg::BinSpec spec = {lg::FRAME_SURFEL, TH, 0, nullptr, "surfel forward"};
    lg::BinnedFrame bf;
    const int rendered = lg::bin_frame(spec, geom, img.ranges, (size_t)P, width, height, -1, -1, pa.compact != 0, binning_alloc, binning_user,
                                       debug, stream, &bf);
    if (rendered < 0) return rendered;
    const lg::FrameLayout& L = bf.L;
    const lg::BinView& bin = bf.bin;
    const int S = L.S;

    lg::SfFwdArgs fa;
    fa.grid = grid; fa.ranges = img.ranges; fa.point_list = bin.val_a; fa.rec = geom.rec; fa.rowspan = geom.rowspan;
    fa.coltab = img.coltab; fa.rowtab = img.rowtab; fa.bg = background; fa.accum = img.accum; fa.n_contrib = img.n_contrib;
    fa.out_color = out_color; fa.out_others = out_others;
    fa.seg = bin.seg; fa.S = S; fa.seg_len = L.plan.seg_len; fa.flags = bin.flags; fa.R = L.Rp; fa.touched = geom.touched;
    // pass 1 in gated rounds (as the 3-D variant, api.hip run_pass1_rounds), pass 2 over what was walked, combine
    {
        const int* rounds = L.plan.rounds;
        const int nr = L.plan.n_rounds;
        fa.alive = nullptr; fa.front = 0;
        int lo = 0;
        for (int i = 0; i < nr && rounds[i] < S; i++) {
            fa.seg_lo = lo; fa.seg_hi = rounds[i];
            lg::launch_sf_render_pass1(fa, stream);
            fa.alive = bin.alive; fa.front = rounds[i];
            lg::launch_sf_alive(fa, stream);
            lo = rounds[i];
        }
        fa.seg_lo = lo; fa.seg_hi = S;
        lg::launch_sf_render_pass1(fa, stream);
        fa.seg_lo = 0; fa.seg_hi = S;
    }
    lg::prof_mark("render_pass1", stream);
    lg::launch_sf_render_pass2(fa, stream);
    lg::prof_mark("render_pass2", stream);
    lg::launch_sf_combine(fa, stream);
    SF_CHECK("surfel render forward");
    lg::prof_mark("render_combine", stream);
    lg::note_forward((size_t)P, bf.R, L, geom.totals, bin.flags, geom.touched, nullptr, stream);
    return rendered;
}

// lidargs_surfel_backward's host sequence.  dL_dviewmatrix (lgsfpose_backward_view, else NULL): the chain's pose form and the fold of its
// partial rows run in place of the chain (two launches for one), with scale_modifier, which the chain itself does not read.
static int sf_backward_impl(int P, int R, const float* background, int width, int height, const float* means3D, const float* scales,
                            float scale_modifier, const float* rotations, const float* transMat_precomp, const float* viewmatrix,
                            const float* beam_inclinations, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                            const float* dL_dpix, const float* dL_depths, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
                            float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dtransMat_2dtemp, float* dL_dscale,
                            float* dL_drot, float* depth, int debug, hipStream_t stream, float* dL_dviewmatrix, float* view_partials) {
    if (P < 0 || R < 0 || width <= 0 || height < 2) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel backward: bad sizes");
    if (P == 0) return 0;
    // transMat_precomp with scales and rotations: the blend's backward runs on the precomputed rows (they are in the forward's records),
    // the chain to scales / rotations / means3D runs as always (R2/cr/backward.cu:730: Ts_precomp is only set when scales is NULL, and
    // that case -- "Ts_precomp error, to check!!", :661-664 -- cannot get past the forward); dL_dtransMat is what the caller returns for it
    if (!geom_buffer || !binning_buffer || !image_buffer) return lg::api_fail(LIDARGS_ERR_STATE, "surfel backward: missing forward buffers");
    SF_SCENE(sc, beam_inclinations); SF_GRAD_ROWS(rows);
    if (!means3D || !scales || !rotations || !viewmatrix || !beam_inclinations || !background || !radii || !dL_dpix || !dL_depths || !rows.required() || !depth)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel backward: NULL required pointer");
    const lg::FrameLayout L = lg::frame_layout(R, width, height, -1, -1, lg::FRAME_SURFEL);
    lg::GeomView geom; lg::geom_carve(geom_buffer, (size_t)P, lg::SURFEL_BUFFERS, &geom);
    lg::BinView bin; L.bin_carve(binning_buffer, &bin);
    lg::SfImgView img; lg::sf_img_carve(image_buffer, width, height, L.grid.num_tiles(), &img);
    lg::prof_begin(stream, 1);
    lg::launch_zero_touched(geom.touched, reinterpret_cast<float4*>(geom.gacc), 8, (size_t)P, geom.tlist, geom.tcount, rows.zero_rows(), stream);   // the touched surfels' lines + lists, every backward
    lg::prof_mark("bwd_zero", stream);
    lg::SfBwdArgs ba;
    ba.grid = L.grid; ba.ranges = img.ranges; ba.point_list = bin.val_a; ba.rec = geom.rec; ba.rowspan = geom.rowspan;
    ba.coltab = img.coltab; ba.rowtab = img.rowtab; ba.bg = background; ba.accum = img.accum; ba.n_contrib = img.n_contrib;
    ba.dL_dpix = dL_dpix; ba.dL_dothers = dL_depths; ba.gacc = geom.gacc;
    ba.seg = bin.seg; ba.S = L.S; ba.seg_len = L.plan.seg_len; ba.flags = bin.flags; ba.R = L.Rp;
    ba.alive = L.gated ? bin.alive : nullptr;
    lg::launch_sf_render_backward(ba, stream);
    SF_CHECK("surfel render backward");
    lg::prof_mark("render_bwd", stream);
    lg::SfGaussBwdArgs ga = lg::sf_gauss_bwd_args(sc, rows, geom.gacc, geom.tlist, geom.tcount); ga.W = width; ga.H = height; ga.radii = radii; ga.depth = depth;
    if (dL_dviewmatrix) {
        ga.view_partials = view_partials; ga.scale_modifier = scale_modifier;
        lg::launch_sf_gaussian_backward_view(ga, dL_dviewmatrix, stream);
    } else lg::launch_sf_gaussian_backward(ga, stream);
    SF_CHECK("surfel gaussian backward");
    lg::prof_mark("gaussian_bwd", stream);
    return 0;
}

int lidargs_surfel_backward(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                            const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                            const float* rotations, const float* transMat_precomp, const float* viewmatrix, const float* projmatrix,
                            const float* campos, const float* beam_inclinations, const int* radii, char* geom_buffer,
                            char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_depths, float* dL_dmean2D,
                            float* dL_dnormal, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat,
                            float* dL_dtransMat_2dtemp, float* dL_dsh, float* dL_dscale, float* dL_drot, float* depth, int debug,
                            void* stream_) {
    (void)D; (void)M; (void)shs; (void)colors_precomp; (void)projmatrix; (void)campos; (void)dL_dsh;
    return sf_backward_impl(P, R, background, width, height, means3D, scales, scale_modifier, rotations, transMat_precomp, viewmatrix,
                            beam_inclinations, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_depths, dL_dmean2D, dL_dnormal,
                            dL_dopacity, dL_dcolor, dL_dmean3D, dL_dtransMat, dL_dtransMat_2dtemp, dL_dscale, dL_drot, depth, debug,
                            (hipStream_t)stream_, nullptr, nullptr);
}

size_t lgsfpose_view_partial_floats(int P) { return lg::view_partial_floats(P); }

// the pose entry points' own refusals, before lidargs_surfel_backward's: 1 = P == 0 (sixteen zeros queued, return 0), 0 = go on
static int sf_pose_check(const char* who, int P, bool bad_sizes, const float* transMat_precomp, float* dL_dviewmatrix, float* view_partials,
                         size_t view_partial_floats, hipStream_t stream) {
    static thread_local char msg[256];
    const auto refuse = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, msg); };
    if (bad_sizes) return refuse("bad sizes");
    if (!dL_dviewmatrix) return refuse("dL_dviewmatrix is NULL");
    if (transMat_precomp)
        return refuse("transMat_precomp together with dL_dviewmatrix (precomputed rows are in view space already: their dependence on the pose is the caller's, through dL_dtransMat)");
    if (P == 0) {
        SF_HIP(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), stream));
        return 1;
    }
    if (!view_partials || ((uintptr_t)view_partials & 15u) || view_partial_floats < lg::view_partial_floats(P))
        return refuse("view_partials is NULL, not 16-byte aligned or shorter than lgsfpose_view_partial_floats(P)");
    return 0;
}

int lgsfpose_backward_view(int P, int D, int M, int R, const float* background, int width, int height, const float* means3D,
                           const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                           const float* rotations, const float* transMat_precomp, const float* viewmatrix, const float* projmatrix,
                           const float* campos, const float* beam_inclinations, const int* radii, char* geom_buffer,
                           char* binning_buffer, char* image_buffer, const float* dL_dpix, const float* dL_depths, float* dL_dmean2D,
                           float* dL_dnormal, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat,
                           float* dL_dtransMat_2dtemp, float* dL_dsh, float* dL_dscale, float* dL_drot, float* depth, int debug,
                           void* stream_, float* dL_dviewmatrix, float* view_partials, size_t view_partial_floats) {
    (void)D; (void)M; (void)shs; (void)colors_precomp; (void)projmatrix; (void)campos; (void)dL_dsh;
    hipStream_t stream = (hipStream_t)stream_;
    if (const int rc = sf_pose_check("surfel backward_view", P, P < 0 || R < 0 || width <= 0 || height < 2, transMat_precomp, dL_dviewmatrix,
                                     view_partials, view_partial_floats, stream))
        return rc < 0 ? rc : 0;
    return sf_backward_impl(P, R, background, width, height, means3D, scales, scale_modifier, rotations, nullptr, viewmatrix,
                            beam_inclinations, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_depths, dL_dmean2D, dL_dnormal,
                            dL_dopacity, dL_dcolor, dL_dmean3D, dL_dtransMat, dL_dtransMat_2dtemp, dL_dscale, dL_drot, depth, debug, stream,
                            dL_dviewmatrix, view_partials);
}

int lidargs_surfel_visible_filter(lidargs_alloc_fn geometry_alloc, void* geometry_user, lidargs_alloc_fn binning_alloc, void* binning_user,
                                  lidargs_alloc_fn image_alloc, void* image_user, int P, int M, int width, int height, const float* means3D,
                                  const float* scales, float scale_modifier, const float* rotations, const float* transMat_precomp,
                                  const float* viewmatrix, const float* projmatrix, const float* beam_inclinations, int prefiltered,
                                  int lidar_far, int lidar_near, int* radii, int* radii_xy, int debug, void* stream_) {
    (void)geometry_alloc; (void)geometry_user; (void)binning_alloc; (void)binning_user; (void)image_alloc; (void)image_user;
    (void)M; (void)projmatrix; (void)prefiltered;   // (transMat_precomp: the filter's preprocess does not read it)
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || width <= 0 || height < 2) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel visible_filter: bad sizes");
    if (P == 0) return 0;
    if (!means3D || !scales || !rotations || !viewmatrix || !beam_inclinations || !radii || !radii_xy)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "surfel visible_filter: NULL required pointer");
    const lg::TileGrid grid = lg::make_grid(width, height, lg::tile_rows());
    SF_SCENE(sc, beam_inclinations);
    const lg::SfPreArgs pa = lg::sf_pre_params(sc, grid, scale_modifier, (float)lidar_near, (float)lidar_far, radii, radii_xy);
    lg::launch_sf_preprocess(pa, true, stream);
    SF_CHECK("surfel filter preprocess");
    return 0;
}

// Test hooks of the surfel variant's two per-surfel stages: the product's own launchers on caller-supplied arrays; no dispatch is decided here.
int lidargs_debug_surfel_preprocess(int P, int width, int height, const float* means3D, const float* colors, const float* opacities,
                                    const float* scales, float scale_modifier, const float* rotations, const float* transMat_precomp,
                                    const float* viewmatrix, const float* beams, float near_f, float far_f, int tile_rows, int compact, int prune,
                                    int filter_only, float* rec, unsigned* rowspan, unsigned* spans, unsigned* key, unsigned char* touched,
                                    unsigned* totals, int* radii, int* radii_xy, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0 || width <= 0 || height < 2 || height > 65535) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: bad sizes");
    if (tile_rows != 4 && tile_rows != 8 && tile_rows != 16 && tile_rows != 32)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: tile_rows must be 4, 8, 16 or 32");
    const lg::TileGrid grid = lg::make_grid(width, height, tile_rows);
    if (compact && !lg::compact_spans(grid.tiles_x, height))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: compact span records do not hold this image");
    if (transMat_precomp != nullptr && (!scales || !rotations))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: transMat_precomp without scales and rotations");
    if (!means3D || !scales || !rotations || !viewmatrix || !beams || !radii || !radii_xy)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: NULL required pointer");
    if (!filter_only && (!colors || !opacities || !rec || !rowspan || !spans || !key || !touched || !totals))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_preprocess: NULL required pointer");
    if (P == 0) return 0;
    SF_SCENE(sc, beams);
    lg::SfPreArgs pa = lg::sf_pre_params(sc, grid, scale_modifier, near_f, far_f, radii, radii_xy);
    if (!filter_only) {
        lg::GeomView geom; memset(&geom, 0, sizeof geom);
        geom.rec = reinterpret_cast<float4*>(rec); geom.rowspan = rowspan; geom.spans = reinterpret_cast<uint4*>(spans); geom.key_a = key;
        geom.touched = touched; geom.totals = totals;
        lg::sf_pre_outputs(pa, opacities, colors, transMat_precomp, geom, compact ? 1 : 0, prune ? 1 : 0);
        SF_HIP(hipMemsetAsync(totals, 0, LG_TOTALS_WORDS * sizeof(uint32_t), stream));     // as lidargs_surfel_forward does
    }
    lg::launch_sf_preprocess(pa, filter_only != 0, stream);
    SF_CHECK("debug surfel preprocess");
    return 0;
}

int lidargs_debug_surfel_gaussian_backward(int P, int width, int height, int stage, const unsigned char* touched, float* gacc, const float* means3D,
                                           const float* scales, const float* rotations, const float* transMat_precomp, const float* viewmatrix,
                                           const float* beams, const int* radii, float* dL_dmean2D, float* dL_dnormal, float* dL_dopacity,
                                           float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat, float* dL_dtransMat_2dtemp, float* dL_dscale,
                                           float* dL_drot, float* depth, unsigned char* tlist, unsigned short* tcount, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    if (P < 0 || width <= 0 || height < 2) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_gaussian_backward: bad sizes");
    if (stage < 0 || stage > 2) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_gaussian_backward: stage must be 0, 1 or 2");
    if (!touched || !gacc || !tlist || !tcount) return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_gaussian_backward: NULL required pointer");
    const bool chain = stage != 1;
    SF_SCENE(sc, beams); SF_GRAD_ROWS(rows);
    // the chain's rows, as lidargs_surfel_backward requires them (dL_dnormal, dL_dtransMat, dL_dtransMat_2dtemp stay optional)
    if (chain && (!means3D || !scales || !rotations || !viewmatrix || !beams || !radii || !rows.required() || !depth))
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_gaussian_backward: NULL required pointer");
    if (P == 0) return 0;
    if (stage != 2) {
        lg::launch_zero_touched(touched, reinterpret_cast<float4*>(gacc), 8, (size_t)P, tlist, tcount, rows.zero_rows(), stream);
        SF_CHECK("debug surfel zero touched");
    }
    if (!chain) return 0;
    lg::SfGaussBwdArgs ga = lg::sf_gauss_bwd_args(sc, rows, gacc, tlist, tcount); ga.W = width; ga.H = height; ga.radii = radii; ga.depth = depth;
    lg::launch_sf_gaussian_backward(ga, stream);
    SF_CHECK("debug surfel gaussian backward");
    return 0;
}

int lgsfpose_debug_view_backward(int P, int width, int height, const float* gacc, const float* means3D, const float* scales, float scale_modifier,
                                 const float* rotations, const float* viewmatrix, const float* beams, const int* radii, float* dL_dmean2D,
                                 float* dL_dnormal, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dtransMat,
                                 float* dL_dtransMat_2dtemp, float* dL_dscale, float* dL_drot, float* depth, const unsigned char* tlist,
                                 const unsigned short* tcount, float* dL_dviewmatrix, float* view_partials, size_t view_partial_floats,
                                 void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int debug = 0;
    const float* transMat_precomp = nullptr;
    if (const int rc = sf_pose_check("debug_surfel_view_backward", P, P < 0 || width <= 0 || height < 2, transMat_precomp, dL_dviewmatrix,
                                     view_partials, view_partial_floats, stream))
        return rc < 0 ? rc : 0;
    SF_SCENE(sc, beams); SF_GRAD_ROWS(rows);
    if (!gacc || !tlist || !tcount || !means3D || !scales || !rotations || !viewmatrix || !beams || !radii || !rows.required() || !depth)
        return lg::api_fail(LIDARGS_ERR_INVALID_ARGUMENT, "debug_surfel_view_backward: NULL required pointer");
    lg::SfGaussBwdArgs ga = lg::sf_gauss_bwd_args(sc, rows, gacc, tlist, tcount); ga.W = width; ga.H = height; ga.radii = radii; ga.depth = depth;
    ga.view_partials = view_partials; ga.scale_modifier = scale_modifier;
    lg::launch_sf_gaussian_backward_view(ga, dL_dviewmatrix, stream);
    SF_CHECK("debug surfel view backward");
    return 0;
}

}  // extern "C"
