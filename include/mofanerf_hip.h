/*
 * mofanerf_hip.h — C ABI of libmofanerf_hip.so, the MI355X (gfx950) implementation of MoFaNeRF's
 * ray-marching hot path.
 *
 * The reference (zhuhao-nju/mofanerf) is pure Python/PyTorch with no FFI layer; the drop-in boundary
 * is the Python class `myRenderer` (models/render_class.py:40).  This header is what that class's
 * methods bind instead of aten ops.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated; the caller owns every buffer
 *     (PyTorch's caching allocator in the shipped host layer); nothing here allocates or frees.
 *   - `stream` is a hipStream_t passed as void*; no entry point synchronises the host — with ONE exception, mofa_device_init(), the
 *     explicit per-device initialisation (and mofa_prof_end(), which collects a measurement).
 *   - return 0 on success, MOFA_EINVAL for a bad argument, MOFA_EHIP if a launch failed
 *     (hipGetLastError text via mofa_last_error()).
 *   - kernels are stateless and re-entrant per stream.
 *
 * Panel layout ("panels").  Activations and the per-point weight blocks are stored K-panel-major so
 * that one MFMA operand tile is a single contiguous, already bank-swizzled LDS image:
 *     a matrix [rows, K] (K padded to a multiple of 16) is K/16 panels, each [rows][16] floats;
 *     element (row, k) lives at
 *         (k/16)*rows*16 + row*16 + ((((k%16)/4) ^ ((row/4)%4)) * 4) + k%4 .
 * `rows` is the point count padded to 256 for activations, the feature count padded to 64 for weights.
 */
#ifndef MOFANERF_HIP_H
#define MOFANERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden; everything declared in this header — and nothing else — is exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define MOFA_ABI_VERSION 5 /* 2: MofaNetShape carries the encoding / code widths; explicit-point backward; mask tape; no split modes.
                             3: MOFA_PROF_KINDS = 6 (mofa_prof_end's arrays grew by the chained kernel's entry); larger mofa_net_workspace_floats
                             4: mofa_device_init(); `verdict` words of mofa_net_forward / mofa_net_backward; MOFA_PROF_KINDS = 7; larger
                                mofa_net_backward_workspace_floats
                             5: mofa_device_init() runs the chained launch's self-check (third argument); mofa_test_hooks() replaces the two
                                MOFA_CHAIN_* environment hooks; MOFA_PROF_KINDS = 12 (the mask-writing chained forward, the chained training backward and the HBM-bound ray
                                kernels have their own entries); mofa_net_backward_workspace_floats(.., with_weight_grads) */
#define MOFA_OK 0
#define MOFA_EINVAL (-1)
#define MOFA_EHIP (-2)

/* the shipped configuration (configs/exp_mofanerf.txt over tools/config_parser.py:51-56,113-118) — DEFAULTS, not limits:
 * every one of them is a field of MofaNetShape below */
#define MOFA_DEFAULT_PE_POINT_FREQS 10 /* multires       -> 3 + 6*10 = 63 features */
#define MOFA_DEFAULT_PE_VIEW_FREQS 4   /* multires_views -> 3 + 6*4  = 27 features */
#define MOFA_DEFAULT_CH_EXP 30         /* input_ch_expCodes     */
#define MOFA_DEFAULT_CH_SHAPE 50       /* input_ch_shapeCodes   */
#define MOFA_DEFAULT_CH_TEX 256        /* input_ch_textureCodes */
#define MOFA_MAX_PE_FREQS 16           /* 3 + 6*16 = 99 features */
#define MOFA_MAX_CODE 4096
#define MOFA_ROW_TILE 256 /* activation rows are padded to this */

int mofa_abi_version(void);
const char* mofa_last_error(void);   /* thread-local text of the calling thread's last failure */

/* Library-wide state is limited to what is listed here; everything else is in caller-owned buffers.
 *   - five run-time knobs, each choosing between BIT-IDENTICAL forms of the exact-fp32 path — MOFA_GATE=0 (mofa_net_forward_gated runs the
 *     full forward), MOFA_PIPE=0 (plain instead of
 *     software-pipelined K loops), MOFA_FUSED=0/1 (per-layer launches / persistent network kernel for widths <= 256), MOFA_CHAIN=0
 *     (per-layer launches instead of the chained launch of the wider networks), MOFA_CHAIN_TRAIN=1 (the TRAINING backward — products and
 *     weight gradients — as chained launches too; off by default: measured a tie); there is no reduced-precision
 *     mode: read from the environment ONCE when the library is loaded into an immutable snapshot;
 *     no launch path calls getenv.  mofa_config_reload() re-reads them (tests that change a knob inside one process call it explicitly).
 *     Measurement arms (scheduling experiments, time stamps, ablations) are NOT in this library: csrc/measure/, tools/build_measure.py.
 *   - per-device caches (CU count, a one-time function attribute) and the per-device measurement session below. */
int mofa_config_reload(void);

/* TEST HOOKS — for tests/ and tools/ only; the shipped host layer never calls this, and NOTHING in the environment reaches these
 * settings (round 5 read two of them from MOFA_CHAIN_* variables: a stray variable in production turned every wide-network launch into
 * NaN + MofaError).  Process-wide, effective from the next launch / the next mofa_device_init():
 *   chain_spin_limit  polls before a dependency wait of the chained launch (k_net_chain) gives up; 0 = the shipped budget (2^22 polls,
 *                     seconds).  1 forces the "wait out of budget" path: the launch ends incomplete -> NaN outputs + verdict.
 *   chain_skip_xcd    -1 (none), or 0..7: the chained launch's workgroups on that XCD leave at once — what a CU-masked stream that
 *                     starves an XCD looks like (an unworked tile queue -> NaN outputs + verdict "tiles missing").
 *   selfcheck_poison  non-zero: mofa_device_init()'s self-check sees one flipped bit in the chained result (forces its fallback). */
int mofa_test_hooks(uint32_t chain_spin_limit, int32_t chain_skip_xcd, int32_t selfcheck_poison);
/* TEST HOOK: non-zero = chain_spin_limit / chain_skip_xcd reach only the colour launch of mofa_net_forward_gated (the launch over a device-side
 * row-tile count), so that its own verification can be seen to flag it; 0 restores the default (every chained launch). */
int mofa_test_hooks_colour_only(int32_t on);

/* Per-device initialisation — the ONE entry point that allocates (scratch of the checks below, ~70 MB, freed again; plus eight bytes kept
 * per device: the measurement session's device-side FLOP sum, which mofa_prof_begin zeroes and mofa_prof_end reads) and synchronises
 * `stream`.  Call it once per device before the first mofa_net_forward (the shipped host layer does, when a network is bound to a
 * device).  It decides whether the wide networks of this device may take the chained launch (k_net_chain) — two checks, both needed:
 *   1. the XCD census: one tile queue per XCD, so all eight must receive workgroups of a 2-per-CU launch.
 *      xcd_workgroups: NULL, or 8 ints receiving the census.
 *   2. the SELF-CHECK (ABI 5): the chained launch replaces launch boundaries by an inter-workgroup protocol whose visibility leg
 *      (a producer's plain stores, acknowledged by the XCD's L2, are what the consumer's `sc1` loads return) is a property of this
 *      part, not a language guarantee — and the verification kernel behind every chained launch sees incompleteness, not staleness.
 *      So it is checked here: a fixed 10 x 512 network on 4,096 points (16 row tiles: nearly every tile waits on a dependency) runs
 *      twice chained and twice per layer through one recycled workspace and the outputs are compared bit for bit on the device
 *      (~4 ms).  chain_selfcheck: NULL, or receives 1 (identical), 0 (any difference / NaN / incomplete launch: this device takes the
 *      per-layer launches, mofa_last_error() says why), -1 (not run: the census already said no).
 * It also sets the persistent kernel's LDS attribute.  Returns MOFA_OK whenever the device is usable — a failed check is a fallback
 * (per-layer launches: bit-identical, ~1 % slower), not an error.  Without this call the wide networks run per layer too;
 * mofa_net_forward / mofa_net_backward themselves never allocate or synchronise. */
int mofa_device_init(void* stream, int32_t* xcd_workgroups, int32_t* chain_selfcheck);

/* Launch verdicts.  A chained launch (k_net_chain) replaces launch boundaries by an inter-workgroup protocol; if that protocol ever
 * fails — a dependency wait out of budget, a tile queue nobody worked (CU-masked stream) — the kernel does NOT compute on incomplete
 * inputs: the launch ends incomplete, a verification kernel behind it overwrites the call's outputs (raw_out; the gradients) with NaN
 * and raises these words.  `verdict`: NULL, or MOFA_VERDICT_WORDS uint32 on the device, zeroed ONCE by the caller and then sticky:
 *   [0] bit 0 = a wait timed out, bit 1 = tiles missing (0 = every chained launch so far was complete)
 *   [1] chained launches verified   [2] [3] [4] the last launch's flags / finished tiles / expected tiles   [5] bad launches.
 * The host reads them back whenever it likes (asynchronously in the shipped layer) — [0] != 0 is an error, never a result. */
#define MOFA_VERDICT_WORDS 8

/* ---- network description -------------------------------------------------------------------
 * NeRF(D, W, input_ch, input_ch_views, input_ch_textureCodes, input_ch_shapeCodes, use_viewdirs=True, skips=[4]) of
 * models/model.py:80-137 as tools/create_model_condition.py:16-34 builds it from the flags of tools/config_parser.py:51-56,113-118:
 *   input_ch       = (3 + 6*multires) + input_ch_expCodes      (get_embedder, models/model.py:48-63; i_embed = -1: multires -> 0)
 *   input_ch_views =  3 + 6*multires_views
 * `weights`/`biases` are the 2D+7 Linear layers in state-dict order (mofanerf_amd/schema.py::nerf_layers):
 *   xyzEncode.linears1.Linear0..3, linear_BiM_xyz.linears1.Linear0..4, .linears2.Linear0..D-6,
 *   linear_uv_xyzBiM.linears1.Linear0..4, .linears2.Linear0..D-6, linear_view_xyBMuv.0,
 *   alpha_linear.0, rgb_linear — each weight row-major [out, in] exactly as PyTorch stores it; mofa_net_layer_dims() states the
 * [out, in] every entry point below assumes for layer li, so a host layer can REFUSE a module that does not match. */
typedef struct MofaNetShape {
    int32_t D;              /* netdepth  (8 coarse / 10 fine)   */
    int32_t W;              /* netwidth  (256 coarse / 1024 fine) */
    int32_t pe_point_freqs; /* multires       (0 .. MOFA_MAX_PE_FREQS; 0 = the raw coordinates only, i_embed = -1) */
    int32_t pe_view_freqs;  /* multires_views (same range) */
    int32_t ch_exp;         /* expression-code columns behind the point encoding in xyzEncode.Linear0 (0 .. MOFA_MAX_CODE) */
    int32_t ch_shape;       /* shape-code columns in front of linear_BiM_xyz.linears{1,2}.Linear0 */
    int32_t ch_tex;         /* texture-code columns in front of linear_uv_xyzBiM.linears{1,2}.Linear0 */
} MofaNetShape;

int mofa_net_num_layers(MofaNetShape s);          /* 2D+7, or MOFA_EINVAL for an unsupported shape */
int mofa_net_layer_dims(MofaNetShape s, int32_t li, int32_t* n_out, int32_t* n_in);   /* PyTorch weight shape of layer li */
int mofa_pe_k_padded(int32_t n_freqs);            /* roundup(3 + 6*n_freqs, 64): K of the first layer's operand panels */
size_t mofa_net_packed_floats(MofaNetShape s);    /* size of the packed per-point weight blob */
size_t mofa_net_folded_floats(MofaNetShape s);    /* size of the per-call folded-bias blob    */
size_t mofa_net_workspace_floats(MofaNetShape s, int64_t n_points, int64_t n_rays);

/* Repack the per-point-varying weight columns of every layer into panels (+ dense head rows).
 * Replaces nothing in the reference (it multiplies the concatenated inputs, model.py:129-133); the
 * split is exact algebra — see SURVEY.md §7 "constant folding". */
int mofa_net_pack(MofaNetShape s, const float* const* weights, float* packed, void* stream);

/* Per-call folded biases: b' = b + W[:, const cols] @ code for the five conditioned layers
 * (expression [ch_exp] -> xyzEncode.L0; shape [ch_shape] -> BiM l1.L0 / l2.L0; texture [ch_tex] -> uv l1.L0 / l2.L0),
 * plus plain copies of every other bias.  Replaces the torch.cat of expanded codes in
 * render_class.py:74-85,104 and model.py:129,132.   exp_code is the ALREADY modulated code
 * (scale*sigma+bias, render_class.py:81).  A code of width 0 may be NULL. */
int mofa_net_fold(MofaNetShape s, const float* const* weights, const float* const* biases,
                  const float* exp_code, const float* shape_code, const float* tex_code, float* folded,
                  void* stream);

/* run_network + NeRF.forward for n_rays*S points (render_class.py:69-94, model.py:121-137):
 * positional encoding of pts = o + d*z (separately rounded mul and add, render_class.py:315),
 * 2D+5 fused Linear+bias+ReLU layers on MFMA, per-ray view-direction bias, sigma/rgb heads.
 *   rays_o, rays_d, viewdirs [n_rays,3]; z [n_rays,S] (z_row_stride = S) or one shared row (stride 0)
 *   pts: optional explicit [n_rays*S,3] points (then rays_o/rays_d/z may be NULL)
 *   view_w [W/2, (3+6*multires_views)+W], view_b [W/2]: the ORIGINAL linear_view_xyBMuv.0 tensors (their view-encoding
 *   columns become a per-ray bias, computed here from viewdirs)
 *   raw_out [n_rays,S,4] = (rgb pre-sigmoid, sigma pre-ReLU)
 *   workspace: mofa_net_workspace_floats(s, n_rays*S, n_rays) floats.
 *   tape: NULL, or mofa_net_tape_floats() floats that receive EVERY layer's output for mofa_net_backward WITH weight gradients
 *         (training; sized for 288 GB of HBM: no recomputation).  tape == mask_tape == NULL: inference, 4 recycled buffers.
 *   mask_tape: NULL, or mofa_net_mask_tape_words() 64-bit words that receive ONE BIT per layer output, (output > 0) — all the
 *         backward needs when no weight gradient is asked for (fitting: run_fit.py:305-313 never steps the networks).  The
 *         activations themselves are recycled as in inference: 1/32 of the tape, no recomputation.  Excludes `tape`.
 *   view_bias_rows: NULL (computed here from viewdirs), or caller-provided per-ray bias rows [n_rays, roundup(W/2,64)]
 *         (the autograd path computes them on the host so that gradients reach viewdirs and the 27 view columns)
 *   verdict: NULL or the caller's sticky launch-verdict words (above). */
int mofa_net_forward(MofaNetShape s, const float* packed, const float* folded, const float* view_w,
                     const float* view_b, const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride,
                     const float* pts, const float* viewdirs, int64_t n_rays, int32_t S, float* workspace,
                     float* raw_out, float* tape, uint64_t* mask_tape, const float* view_bias_rows, uint32_t* verdict, void* stream);
/* The sigma-gated forward (inference): mofa_net_forward's raw_out with the colour half of the network — texture stack, view layer, rgb
 * head — run only for the samples whose raw density is not <= 0 (NaN counts as live).  A sample with sigma <= 0 has alpha = 0 and weight 0
 * exactly, so compositing never sees its colour: raw_out[..., 3] holds mofa_net_forward's bits everywhere, raw_out[..., 0:3] holds them on
 * the live samples and (0, 0, 0) on the others, and every composited output is the same bits.  Only the chained launch is gated: the geometry
 * half over all rows, a 64-bit scan of the flags, a gather of the live rows' sigmaCodes and view-bias rows, a second chained launch over the
 * live row tiles (a count that stays on the device), the rgb head and a scatter that writes every rgb element.  No tape, no host
 * synchronisation, no allocation.  When the call would not take the chained launch (MOFA_CHAIN=0, MOFA_GATE=0, no or a failed
 * mofa_device_init, widths the chain refuses, the persistent kernel of widths <= 256) it runs mofa_net_forward unchanged.
 *   workspace: mofa_net_forward_gated_workspace_floats(s, n_rays*S, n_rays) floats, 16-byte aligned like raw_out — asked on the device
 *   and under the knobs of the call: it is mofa_net_workspace_floats' figure when the call cannot gate there (knobs, shape, census).
 *   stats: NULL, or two uint64 on the device: [0] += samples, [1] += live samples of every gated call (never read by the library).
 *   gated: receives 1 (the gated route ran) or 0 (the full forward ran).  Everything else as for mofa_net_forward. */
size_t mofa_net_forward_gated_workspace_floats(MofaNetShape s, int64_t n_points, int64_t n_rays);
int mofa_net_forward_gated(MofaNetShape s, const float* packed, const float* folded, const float* view_w, const float* view_b,
                           const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, const float* pts,
                           const float* viewdirs, int64_t n_rays, int32_t S, float* workspace, float* raw_out, const float* view_bias_rows,
                           uint64_t* stats, int32_t* gated, uint32_t* verdict, void* stream);
/* Density only — the geometry half of the network: sigma_out[n] = the pre-ReLU alpha head at explicit points pts [n,3], the SAME bits as
 * raw_out[..., 3] of mofa_net_forward on those points, whatever view directions and texture code that call had.  Density depends on the
 * point, the shape code and the expression code only (model.py:121-128): the launch stops after the linear_BiM_xyz stack — no texture
 * stack, no view layer, no rgb head — on the same layer kernels, chained or per layer by the same choice (never the persistent kernel:
 * widths <= 256 take the per-layer launches, bit-identical).  `folded` from mofa_net_fold (the texture code is not read: zeros do).
 *   workspace: mofa_net_workspace_floats(s, n_points, 1) floats.  verdict: as for mofa_net_forward (a chained launch that ended
 *   incomplete leaves NaN in sigma_out and raises the words). */
int mofa_net_density(MofaNetShape s, const float* packed, const float* folded, const float* pts, int64_t n_points, float* workspace,
                     float* sigma_out, uint32_t* verdict, void* stream);

/* ---- geometry export: grid points and the iso-surface of a density grid ---------------------------------------------------------
 * Grid sample points: pts[n,3] for the flat indices first .. first+n-1 of an nx x ny x nz grid, idx = (i*ny + j)*nz + k (C order, z
 * fastest); x = lo_x + (float)i * step_x with the multiply and the add rounded separately (likewise y, z).  lo / step: HOST arrays. */
int mofa_grid_points(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], int64_t first, int64_t n, float* pts,
                     void* stream);
/* Marching tetrahedra on the Freudenthal split of grid [nx,ny,nz] (the sample at idx above): a watertight, consistently oriented
 * triangle mesh of {sigma >= level} (NaN counts as outside), normals (v1-v0) x (v2-v0) toward lower sigma.  Each cell (i,j,k) is
 * 6 tets {0, e_a, e_a+e_b, e_a+e_b+e_c}, one per axis permutation (a,b,c) in lexicographic order; every tet edge is a lattice edge
 * in one of the directions +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z, owned by its lower endpoint: edge_id = 7 idx + dir.  A vertex sits on
 * every edge whose ends differ, at t = (level - s_a) / (s_b - s_a), p = p_a + t (p_b - p_a) (a = the lower endpoint, p from the
 * mofa_grid_points formula, every operation separately rounded).  Vertices are numbered in increasing edge_id, faces ordered by cell,
 * tet, triangle: no atomics, the same bits on every run.  Two phases, because the caller sizes the outputs:
 *   mofa_iso_count  writes counts[0] = V, counts[1] = F (int64, DEVICE) and keeps the edge / cell scans in `workspace`;
 *   mofa_iso_emit   with the SAME grid, level and workspace afterwards: verts [V,3] (float), faces [F,3] (int32 vertex ids).
 * The grid needs >= 2 samples per axis and 7 nx ny nz < 2^31; the level must be finite; emit needs finite lo and step > 0 (host arrays).
 * A result with V or F above 2^31 - 1 is refused: emit then writes nothing (the caller sees it in the counts).  V = F = 0 is a result.
 * A non-finite sample next to a crossing gives non-finite vertices: check the grid first. */
size_t mofa_iso_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);   /* 0 for a grid that is refused */
int mofa_iso_count(const float* grid, int64_t nx, int64_t ny, int64_t nz, float level, void* workspace, int64_t* counts, void* stream);
int mofa_iso_emit(const float* grid, int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], float level, void* workspace,
                  float* verts, int32_t* faces, void* stream);

/* Narrow-band ("sparse brick") extraction: the mesh of mofa_iso_count / mofa_iso_emit on the same fine lattice (the grid above with
 * lo / step), with densities asked for only in bricks the surface passes through.  brick = B in {4, 8, 16}, and (n - 1) % B == 0 on every
 * axis; brick (bi,bj,bk) covers the cells [bi B, (bi+1) B) per axis (index (bi * by + bj) * bz + bk, b_a = (n_a - 1) / B bricks per axis)
 * and samples its (B+1)^3 lattice points, local l = (li (B+1) + lj) (B+1) + lk, global i = bi B + li.  Inside, edges, edge_id, vertex
 * arithmetic and orientation are those of mofa_iso_*; a point evaluated twice must give the same bits (the density is a function of the
 * point).  The caller drives the rounds and supplies every density:
 *   seed   the brick-corner lattice, corner c = (ci (by+1) + cj) (bz+1) + ck at lattice point (ci B, cj B, ck B)
 *          (mofa_band_corner_points); mofa_band_seed activates every brick whose 8 corners are not all on one side of the level;
 *   round  mofa_band_points gives the (B+1)^3 points of each brick just activated (n_new = counts[0] of the last seed / grow, point
 *          p = q (B+1)^3 + l of the q-th of them); the caller writes their densities to sigma[(n_active - n_new) (B+1)^3 + p]
 *          (n_active = counts[1]; sigma keeps every earlier round's densities); mofa_band_grow then activates every neighbour brick
 *          (across a face, edge or corner) that an outer-layer cell (local index 0 or B-1 on some axis) with a triangle of those bricks
 *          touches; repeat while counts[0] > 0;
 *   mesh   mofa_band_count (V, F) and mofa_band_emit, as for mofa_iso_*.
 * Every connected component of the iso-surface (connected through shared crossing edges) that passes through a seeded brick is
 * extracted completely and exactly; a component inside bricks whose corners do not straddle the level is missed.  Vertices come by
 * active brick (ascending index), then by edge_id within the brick (a lattice point belongs to brick min(i / B, b_a - 1) per axis and
 * owns the edges leaving it); faces by brick, cell (C order within the brick), tet, triangle; edge_ids[v] is the vertex's edge_id, so
 * ordering the vertices by it gives mofa_iso_emit's numbering.  No atomics: the same bytes on every run and at every chunk size.
 * Memory: the band workspace is O(1) per brick of the brick grid; the mesh workspace and sigma grow with the active bricks only.
 * Every count is written to DEVICE memory (int64).  lo / step: HOST arrays (finite, step > 0).  The level must be finite.  The grid
 * needs 2 <= n < 2^24 per axis and fewer than 2^31 brick corners.  mofa_band_count and mofa_band_emit read the workspace's active count
 * back (a host synchronisation) and return MOFA_EINVAL unless n_active equals it; mofa_band_emit also reads V and F back and returns
 * MOFA_EINVAL, writing nothing, when either exceeds 2^31 - 1. */
size_t mofa_band_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, int32_t brick);   /* 0 for a grid / brick that is refused */
size_t mofa_band_mesh_bytes(int32_t brick, int64_t n_active);                          /* 0 for n_active < 1 or a bad brick */
int mofa_band_corner_points(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], int64_t first, int64_t n,
                            float* pts, void* stream);                       /* pts[n,3]: corners first .. first+n-1 */
/* corner_sigma[(b_x+1)(b_y+1)(b_z+1)]: counts[0] = seeded bricks (the first round's list), counts[1] = active bricks */
int mofa_band_seed(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* corner_sigma, float level, void* workspace, int64_t* counts,
                   void* stream);
int mofa_band_points(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], const void* workspace,
                     int64_t n_new, int64_t first, int64_t n, float* pts, void* stream);   /* points first .. first+n-1 of the round */
/* n_new: the host's copy of the last counts[0]; counts[0] = bricks added (the next round's list), counts[1] = active bricks */
int mofa_band_grow(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* sigma, float level, void* workspace, int64_t n_new,
                   int64_t* counts, void* stream);
/* after the last round (n_active = the last counts[1] >= 1, mesh_workspace of mofa_band_mesh_bytes(brick, n_active)): counts[0] = V,
 * counts[1] = F; bricks (DEVICE int64[n_active], may be NULL) = the active brick indices in ascending order */
int mofa_band_count(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float* sigma, float level, void* workspace, int64_t n_active,
                    void* mesh_workspace, int64_t* counts, int64_t* bricks, void* stream);
/* with the SAME sigma, level and workspaces afterwards: verts [V,3] (float), edge_ids [V] (int64), faces [F,3] (int32 vertex ids) */
int mofa_band_emit(int64_t nx, int64_t ny, int64_t nz, int32_t brick, const float lo[3], const float step[3], const float* sigma, float level,
                   const void* workspace, int64_t n_active, const void* mesh_workspace, float* verts, int64_t* edge_ids, int32_t* faces,
                   void* stream);

/* Vertex refinement: every vertex of mofa_iso_emit / mofa_band_emit keeps its lattice edge and moves along it by a bracketed bisection on
 * the density itself, and density normals come from central differences.  The kernels make sample points and consume densities; the
 * caller evaluates the density in between (a point evaluated twice must give the same bits, as for the narrow band).  Faces, vertex
 * numbering and topology are untouched.  Plain fp32, every operation rounded separately; no atomics but the error counters
 * counts[MOFA_REFINE_COUNTS] (int64, DEVICE), which the CALLER zeroes and the kernels add to, so the same input gives the same bits.
 *   mofa_iso_edge_ids        after mofa_iso_count on the same workspace: edge_ids[V] (int64) = the edge_id of every vertex in
 *                            mofa_iso_emit's order (mofa_band_emit returns its own).  Writes nothing when V or F exceeds 2^31 - 1.
 *   mofa_edge_points         pts[n,3] for the vertices first .. first+n-1 (edge_ids, t_lo, t_hi are indexed by vertex, pts by vertex - first):
 *                            mode 0 the edge's lower end p_a, mode 1 its upper end p_b (both the bits of mofa_grid_points), mode 2 the
 *                            bracket's midpoint p_a + t_m (p_b - p_a), t_m = 0.5 (t_lo + t_hi) (exact for 23 halvings).  t_lo / t_hi may
 *                            be NULL for modes 0 and 1.  An edge id outside [0, 7 nx ny nz) or an edge that leaves the grid adds one to
 *                            counts[MOFA_REFINE_REFUSED] and its point is not written.
 *   mofa_edge_bracket_init   t_lo = 0, t_hi = 1, s_lo = s_a, s_hi = s_b (the densities at p_a, p_b); counts[MOFA_REFINE_NO_STRADDLE] +=
 *                            edges whose ends lie on one side of the level (inside(s) = s >= level, NaN outside),
 *                            counts[MOFA_REFINE_NON_FINITE] += non-finite values.
 *   mofa_edge_bracket_update s_m = the densities at the midpoints: inside(s_m) == inside(s_lo) ? (t_lo, s_lo) = (t_m, s_m) :
 *                            (t_hi, s_hi) = (t_m, s_m).  A non-finite s_m adds one to counts[MOFA_REFINE_NON_FINITE] and leaves its bracket.
 *   mofa_edge_place          u = (level - s_lo) / (s_hi - s_lo), t = t_lo + u (t_hi - t_lo), verts[v] = p_a + t (p_b - p_a).  With an
 *                            untouched bracket t = u: mofa_iso_emit's vertex, bit for bit.  Refused edges as for mofa_edge_points.
 *   mofa_fd_points           pts[6n,3] for the vertices first .. first+n-1 of verts: v + h_x e_x, v - h_x e_x, then y, then z.
 *   mofa_fd_normals          s[6n] = the densities at those points: g_a = (s_+ - s_-) / (2 h_a) in fp32, normals[v] = -g / |g| with the norm
 *                            and the division in fp64 from the three fp32 components, rounded once (toward lower density, like the face
 *                            normals).  A zero or non-finite g gives (0, 0, 0) and adds one to counts[MOFA_REFINE_ZERO_NORMAL].
 * The lattice needs 2 <= n < 2^24 per axis and fewer than 2^48 samples; lo / step / h: HOST arrays (finite, step > 0, h > 0); the level
 * must be finite; 1 <= n <= (2^31 - 1) 256 elements per call. */
#define MOFA_REFINE_NO_STRADDLE 0
#define MOFA_REFINE_NON_FINITE 1
#define MOFA_REFINE_REFUSED 2
#define MOFA_REFINE_ZERO_NORMAL 3
#define MOFA_REFINE_COUNTS 4
int mofa_iso_edge_ids(int64_t nx, int64_t ny, int64_t nz, const void* workspace, int64_t* edge_ids, void* stream);
int mofa_edge_points(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], const int64_t* edge_ids, const float* t_lo,
                     const float* t_hi, int64_t first, int64_t n, int32_t mode, float* pts, int64_t* counts, void* stream);
int mofa_edge_bracket_init(const float* s_a, const float* s_b, float level, int64_t n, float* t_lo, float* t_hi, float* s_lo, float* s_hi,
                           int64_t* counts, void* stream);
int mofa_edge_bracket_update(const float* s_m, float level, int64_t n, float* t_lo, float* t_hi, float* s_lo, float* s_hi, int64_t* counts,
                             void* stream);
int mofa_edge_place(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], const int64_t* edge_ids, const float* t_lo,
                    const float* t_hi, const float* s_lo, const float* s_hi, float level, int64_t n, float* verts, int64_t* counts,
                    void* stream);
int mofa_fd_points(const float* verts, const float h[3], int64_t first, int64_t n, float* pts, void* stream);
int mofa_fd_normals(const float* s, const float h[3], int64_t n, float* normals, int64_t* counts, void* stream);

/* Connected components of a triangle mesh (verts [V,3] float, faces [F,3] int32; 1 <= V, F <= 2^31 - 1): two faces belong to one
 * component when they share a vertex INDEX; a degenerate face (a, a, b) still joins a and b.  The caller (mesh.py) drives the passes.
 * Every kernel checks the indices it dereferences (a face with an index outside [0, V) is skipped), so a bad index is never a GPU fault;
 * mofa_cc_validate is how the caller learns of one before anything else runs.  No kernel waits on another thread: the only loop whose
 * trip count depends on the data is the root walk x = parent[x], which strictly decreases.  Integer atomicMin on parent[] is the only
 * atomic besides the validation's error counter, so the same mesh gives the same bits every time.
 *   mofa_cc_validate    counts[0] (int64, DEVICE, zeroed by the caller) += the face indices outside [0, V)
 *   mofa_cc_init        parent[v] = v (int32 [V])
 *   mofa_cc_hook        for the edges (a, b) and (b, c) of every face: ra = root(a), rb = root(b); if they differ,
 *                       atomicMin(&parent[max(ra, rb)], min(ra, rb)) and *changed = 1 (int64, DEVICE, zeroed by the caller)
 *   mofa_cc_compress    parent[v] = root(v).  hook + compress are repeated until a pass leaves *changed at 0: then parent[v] is the
 *                       smallest vertex index of v's component
 *   mofa_cc_face_terms  terms [F,2] (double), each operation rounded separately in fp64 from the fp32 coordinates:
 *                       terms[f][0] = 0.5 |(v1 - v0) x (v2 - v0)|, terms[f][1] = v0 . (v1 x v2) / 6
 *   mofa_cc_seg_sum     out [n_segments,2] (double): out[s] = the sum of the rows seg_start[s] .. seg_end[s] - 1 (int64, DEVICE, clipped to
 *                       [0, N)) of in [N,2], read through perm [N] (int64, DEVICE; NULL = the identity) — one workgroup per segment, a fixed
 *                       order and a fixed tree, the same bits every time.  longest >= every segment's length (rows beyond it are not summed).
 *   mofa_cc_seg_minmax  out [n_segments,2,3] (float) = the exact [min xyz, max xyz] over each segment's rows of in — points [N,3] (boxes = 0)
 *                       or boxes [N,2,3] (boxes != 0) —, walked like mofa_cc_seg_sum; floats are compared by their order-preserving integer
 *                       key (-0 < +0).  An empty segment gets NaN.
 *   mofa_cc_remap       out[i] = vmap[in[i]] for n int32 indices (vmap int32 [V]); -1 for an index outside [0, V) */
int mofa_cc_validate(const int32_t* faces, int64_t F, int64_t V, int64_t* counts, void* stream);
int mofa_cc_init(int32_t* parent, int64_t V, void* stream);
int mofa_cc_hook(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int64_t* changed, void* stream);
int mofa_cc_compress(int32_t* parent, int64_t V, void* stream);
int mofa_cc_face_terms(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* terms, void* stream);
int mofa_cc_seg_sum(const double* in, const int64_t* perm, int64_t N, const int64_t* seg_start, const int64_t* seg_end, int64_t n_segments,
                    int64_t longest, double* out, void* stream);
int mofa_cc_seg_minmax(const float* in, int32_t boxes, const int64_t* perm, int64_t N, const int64_t* seg_start, const int64_t* seg_end,
                       int64_t n_segments, int64_t longest, float* out, void* stream);
int mofa_cc_remap(const int32_t* in, int64_t n, const int32_t* vmap, int64_t V, int32_t* out, void* stream);

/* Mesh simplification: vertex clustering on a lattice of cells, one quadric-error representative per cluster (mesh.py drives the passes:
 * mesh.simplify; 1 <= V, F, C <= 2^31 - 1, anything indexed by 3 F is 64-bit).  No float or double atomics: sums are fixed-order, fixed-tree
 * segmented reductions, so the same mesh gives the same bits every time; the only atomics are the integer counters counts[MOFA_SIMP_COUNTS]
 * (int64, DEVICE, zeroed by the caller).  Every kernel checks the indices it dereferences: a bad one is counted in
 * counts[MOFA_SIMP_BAD_INDEX] and skipped.  No kernel waits on another thread.  All arithmetic has every operation rounded separately.
 *   mofa_simp_keys             keys[v] (int64) = (q_x << 42) | (q_y << 21) | q_z with q_a = floorf((x_a - origin_a) / cell_a) in fp32; a vertex
 *                              with a non-finite coordinate or a q_a outside [0, 2^21) gets -1 and is counted in counts[MOFA_SIMP_BAD_VERTEX]
 *   mofa_simp_corner_quadrics  quadrics [F,10] (double), from the fp32 coordinates in fp64: n = (v1 - v0) x (v2 - v0) (un-normalised: area^2
 *                              weights), d = -((nx v0x + ny v0y) + nz v0z), row = nx nx, nx ny, nx nz, ny ny, ny nz, nz nz, nx d, ny d, nz d, d d.
 *                              The quadric of face f belongs to the cluster of each of its corners: pair 3 f + c.  The 3 F pairs are not
 *                              materialised; mofa_simp_seg_sum gathers row perm[i] / 3 (80 F bytes instead of 240 F).
 *   mofa_simp_seg_sum          out [n_segments, ncols] (double; ncols = 4 or 10): out[s] = the sum over i in [seg_start[s], seg_end[s]) of row
 *                              perm[i] / row_div of in [N, ncols] (perm int64 [N row_div], DEVICE; NULL = the identity, row_div = 1): one
 *                              workgroup per segment, thread t adds i = s0 + t, s0 + t + 256, ... in that order from +0.0, then the tree
 *                              sm[t] += sm[t + w] (t < w) for w = 128, 64, ..., 1.  longest >= every segment's length.
 *   mofa_simp_place            out [C,3] (float), one representative per cluster from its summed quadric Q [C,10] and S [C,4] = the sum of
 *                              (x, y, z, 1) over its vertices, in fp64 in this order:
 *                                m_a = S_a / S_3;  w = regularize ((Q0 + Q3) + Q5);  a00 = Q0 + w, a11 = Q3 + w, a22 = Q5 + w, a01 = Q1, a02 = Q2,
 *                                a12 = Q4;  r_a = w m_a - Q(6 + a);  c00 = a11 a22 - a12 a12, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11,
 *                                c11 = a00 a22 - a02 a02, c12 = a01 a02 - a00 a12, c22 = a00 a11 - a01 a01;  det = (a00 c00 + a01 c01) + a02 c02;
 *                                x_0 = ((c00 r0 + c01 r1) + c02 r2) / det, x_1 = ((c01 r0 + c11 r1) + c12 r2) / det, x_2 = ((c02 r0 + c12 r1) + c22 r2) / det
 *                              (float) x is taken iff w > 0, w and det finite, det > 0 and mofa_simp_keys' arithmetic on it gives cluster_keys[c];
 *                              otherwise (float) m under the same key test; otherwise verts[first[c]].  mode MOFA_SIMP_PLACE_MEAN starts at
 *                              the mean (quadrics may be NULL).  counts[MOFA_SIMP_QUADRIC / _MEAN / _FIRST] += the route taken,
 *                              counts[MOFA_SIMP_MEAN_REQUESTED] += the clusters asked to start at the mean.
 *   mofa_simp_faces            out[f] = (cluster[faces[f][c]])_c rotated so that the smallest index comes first (orientation kept);
 *                              degenerate[f] (uint8) = two of the three are equal, or an index was bad (then out[f] = -1 -1 -1) */
enum { MOFA_SIMP_BAD_VERTEX = 0, MOFA_SIMP_QUADRIC = 1, MOFA_SIMP_MEAN = 2, MOFA_SIMP_FIRST = 3, MOFA_SIMP_MEAN_REQUESTED = 4,
       MOFA_SIMP_BAD_INDEX = 5, MOFA_SIMP_COUNTS = 6 };
enum { MOFA_SIMP_PLACE_QUADRIC = 0, MOFA_SIMP_PLACE_MEAN = 1 };
int mofa_simp_keys(const float* verts, int64_t V, const float origin[3], const float cell[3], int64_t* keys, int64_t* counts, void* stream);
int mofa_simp_corner_quadrics(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* quadrics, int64_t* counts, void* stream);
int mofa_simp_seg_sum(const double* in, int32_t ncols, const int64_t* perm, int32_t row_div, int64_t N, const int64_t* seg_start,
                      const int64_t* seg_end, int64_t n_segments, int64_t longest, double* out, void* stream);
int mofa_simp_place(const double* quadrics, const double* vsum, const int64_t* cluster_keys, const int32_t* first, const float* verts, int64_t V,
                    int64_t C, const float origin[3], const float cell[3], double regularize, int32_t mode, float* out, int64_t* counts,
                    void* stream);
int mofa_simp_faces(const int32_t* faces, int64_t F, int64_t V, const int32_t* cluster, int64_t C, int32_t* out, uint8_t* degenerate,
                    int64_t* counts, void* stream);

/* Mesh surface distance: the exact closest point on a triangle mesh (verts [V,3] float, faces [F,3] int32) for N query points through a
 * uniform grid of face lists, and a deterministic quadrature of a surface (mesh.py drives the passes: mesh.closest_points,
 * mesh.sample_faces, mesh.surface_distance; 1 <= N, V, F, P, S <= 2^31 - 1).  No float or double atomics: the same input gives the same
 * bytes every time; the only atomics are the integer counters counts[MOFA_DIST_COUNTS] (int64, DEVICE, zeroed by the caller).  Every kernel
 * checks the indices it dereferences: a bad one is skipped.  No kernel waits on another thread.  All arithmetic is fp64 on the fp32
 * coordinates widened, every operation rounded separately; dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 *   the triangle       closest point q of (a, b, c) to p, in Ericson's region order:
 *                        ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 && d2 <= 0: q = a, bary (1, 0, 0)
 *                        bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp);  d3 >= 0 && d4 <= d3: q = b, bary (0, 1, 0)
 *                        vc = d1 d4 - d3 d2;  vc <= 0 && d1 >= 0 && d3 <= 0: v = d1 / (d1 - d3), q = a + v ab, bary (1 - v, v, 0)
 *                        cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp);  d6 >= 0 && d5 <= d6: q = c, bary (0, 0, 1)
 *                        vb = d5 d2 - d1 d6;  vb <= 0 && d2 >= 0 && d6 <= 0: w = d2 / (d2 - d6), q = a + w ac, bary (1 - w, 0, w)
 *                        va = d3 d6 - d5 d4, e = d4 - d3, g = d5 - d6;  va <= 0 && e >= 0 && g >= 0: w = e / (e + g), q = b + w (c - b),
 *                          bary (0, 1 - w, w)
 *                        s = (va + vb) + vc;  s not finite or s <= 0: the face is skipped for this point (counts[MOFA_DIST_SKIPPED]);
 *                        v = vb / s, w = vc / s, q = (a + v ab) + w ac, bary ((1 - v) - w, v, w)
 *                      then per axis q = q < lo ? lo : q, q = q > hi ? hi : q with lo / hi the smallest / largest of the three vertices
 *                      (the closest point lies in the triangle's box: this removes rounding only), and d2 = ((px - qx)^2 + (py - qy)^2) +
 *                      (pz - qz)^2.  Across faces the smaller d2 wins, among equal d2 the lower face index, a NaN d2 never: the answer is a
 *                      function of the mesh and the point alone.
 *   the grid           n[3] cells (1 .. MOFA_DIST_MAX_GRID per axis, fewer than 2^31 - 1 in all) from origin[3] with cell[3] > 0 (HOST arrays
 *                      of doubles).  The cell of a coordinate x: t = floor((x - origin) / cell), index = t >= 0 ? (t < n ? (int) t : n - 1) : 0;
 *                      cell id = (ix n[1] + iy) n[2] + iz.  A face whose normal ab x ac = (aby acz - abz acy, abz acx - abx acz, abx acy - aby acx)
 *                      is exactly (0, 0, 0) is DEGENERATE: it enters no cell.  Every other face enters every cell of the index box of its
 *                      three vertices.
 *   mofa_dist_validate     counts[0] += the non-finite coordinates of verts
 *   mofa_dist_bin_count    n_cells[f] (int64) = the cells face f enters; counts[MOFA_DIST_DEGENERATE] += the degenerate faces
 *   mofa_dist_bin_emit     with offsets [F] (int64, DEVICE) = the exclusive sum of n_cells and P = its total: pair_cell / pair_face [P] (int32),
 *                          face f's cells in ascending id from offsets[f].  The caller sorts the pairs stably by cell (each cell's faces then
 *                          ascend) and forms cell_start [cells + 1] (int32): the pairs of cell c are cell_start[c] .. cell_start[c + 1] - 1.
 *   mofa_dist_query        one thread per query; thread i takes query order[i] (int64 [N], DEVICE: a permutation that puts queries of one
 *                          cell next to each other; NULL = the identity) and writes its slots of distance [N] (float: sqrt(d2) in fp64,
 *                          rounded once), d2 [N] (double), face [N] (int32), closest [N,3] (float), bary [N,3] (float).  From the cell c of the
 *                          point it visits the cells of Chebyshev ring r = 0, 1, 2, ... (clipped to the grid).  After ring r, for every axis
 *                          and side on which the visited block has not reached the grid's edge (c - r > 0; c + r < n - 1):
 *                            low:  ((p - (origin + (double)(c - r) cell)) - slack) (1 - 2^-40)
 *                            high: (((origin + (double)(c + r + 1) cell) - p) - slack) (1 - 2^-40)
 *                          and lb = the smallest of them: every face not yet seen has d2 > lb^2 when lb > 0 (slack[3] >= 0 covers the rounding
 *                          of the cell arithmetic; DESIGN 3.17 derives how much it takes).  The walk ends when no such side is left, or when
 *                          lb > 0 and (best d2 < lb lb, strictly: an equal d2 with a lower index may sit in the next ring; or lb > max_distance).
 *                          max_distance > 0 (infinity: unbounded): a query whose sqrt(d2) is not <= max_distance, or that found no face,
 *                          gets face -1, distance and d2 +infinity, closest and bary NaN.  A query with a non-finite coordinate gets face -1
 *                          and NaN everywhere and is counted in counts[MOFA_DIST_NON_FINITE].  counts[MOFA_DIST_TESTS] += the point-triangle
 *                          tests, counts[MOFA_DIST_MAX_RING] = max(the last ring of any query): both depend on the grid, no result bit does.
 *                          pair_face may be NULL when P = 0.
 *   mofa_dist_sample_count area[f] (double) = 0.5 sqrt((nx nx + ny ny) + nz nz) of the normal above and k[f] (int32) = ceil(sqrt(L) / spacing)
 *                          clamped to 1 .. max_subdiv (<= MOFA_DIST_MAX_SUBDIV), L = the largest of dot(ab, ab), dot(ac, ac), dot(bc, bc) with
 *                          bc = c - b; a degenerate face gets area 0 and k 0 (no samples)
 *   mofa_dist_sample_emit  with offsets [F] (int64) = the exclusive sum of k^2, S its total and face_of [S] (int32) the face of every sample:
 *                          sample offsets[f] + t is the centroid of sub-triangle t of the regular subdivision of face f into k^2 congruent
 *                          triangles.  Row i = 0 .. k - 1 starts at t = 2 k i - i^2 and holds, for j = 0 .. k - 1 - i, the upright triangle
 *                          (numerators nv = 3 i + 1, nw = 3 j + 1) and, for j < k - 1 - i, after it the inverted one (nv = 3 i + 2,
 *                          nw = 3 j + 2); nu = 3 k - nv - nw.  points[s] = (float)(((nu a + nv b) + nw c) / (3 k)) per axis in fp64,
 *                          weight[s] (double) = area[f] / (double)(k k).  A sample whose face_of / offsets do not fit gets NaN and weight 0. */
enum { MOFA_DIST_DEGENERATE = 0, MOFA_DIST_NON_FINITE = 1, MOFA_DIST_TESTS = 2, MOFA_DIST_MAX_RING = 3, MOFA_DIST_SKIPPED = 4,
       MOFA_DIST_COUNTS = 5 };
#define MOFA_DIST_MAX_GRID 1024
#define MOFA_DIST_MAX_SUBDIV 1024
int mofa_dist_validate(const float* verts, int64_t V, int64_t* counts, void* stream);
int mofa_dist_bin_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double origin[3], const double cell[3],
                        const double slack[3], const int32_t n[3], int64_t* n_cells, int64_t* counts, void* stream);
int mofa_dist_bin_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double origin[3], const double cell[3],
                       const double slack[3], const int32_t n[3], const int64_t* offsets, int64_t P, int32_t* pair_cell, int32_t* pair_face,
                       void* stream);
int mofa_dist_query(const float* points, int64_t N, const int64_t* order, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    const double origin[3], const double cell[3], const double slack[3], const int32_t n[3], const int32_t* cell_start,
                    const int32_t* pair_face, int64_t P, double max_distance, float* distance, double* d2, int32_t* face, float* closest,
                    float* bary, int64_t* counts, void* stream);
int mofa_dist_sample_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, double spacing, int32_t max_subdiv, double* area,
                           int32_t* k, void* stream);
int mofa_dist_sample_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, const double* area, const int32_t* k,
                          const int64_t* offsets, const int32_t* face_of, int64_t S, float* points, double* weight, void* stream);

/* Mesh winding numbers: the signed count of the faces of a triangle mesh (verts [V,3] float, faces [F,3] int32) that the ray p + t e_a,
 * t > 0, of a query p crosses, for N queries through a 2-D grid of face lists (mesh.py drives the passes: mesh.winding_number,
 * mesh.signed_distance, mesh.surface_distance(signed=True), mesh.inside_grid; 1 <= N, V, F <= 2^31 - 1, axis a = 0, 1 or 2).  For a closed
 * mesh the count is the winding number of the surface around p: +1 inside a solid whose normals point outward, 0 outside and in a cavity,
 * 2 inside two overlapping solids, -1 inside an inward-oriented mesh.  No float or double atomics: the same input gives the same bytes every
 * time; the only atomics are the integer counters counts[MOFA_WIND_COUNTS] (int64, DEVICE, zeroed by the caller).  Every kernel checks the
 * indices it dereferences: a bad one is skipped.  No kernel waits on another thread.  With u = (a + 1) % 3 and v = (a + 2) % 3 ((u, v, a)
 * is right-handed), all arithmetic is fp64 on the fp32 coordinates widened, every difference and every product rounded separately (no FMA).
 *   the face           (X0, X1, X2) against p:
 *                        1. right_k = X_k.u > p.u.  All three equal: the face is not crossed.
 *                        2. The edge X_k -> X_k+1 straddles when right_k != right_k+1; L = its non-right endpoint, R = its right one (the
 *                           same points in the same roles for the two faces of an edge: both compute the same bits).
 *                             p.v >= max(L.v, R.v): not above;  p.v < min(L.v, R.v): above;  otherwise
 *                             E = (R.u - L.u) (p.v - L.v) - (R.v - L.v) (p.u - L.u), above = E < 0 (a tie is not above).
 *                           An edge that is above adds right_k ? +1 : -1 to w.  Zero or two edges straddle: w is -1, 0 or +1.
 *                        3. Only when w != 0:  p.a < min X_k.a: hit;  p.a >= max X_k.a: no hit;  otherwise ab = X1 - X0, ac = X2 - X0,
 *                           d = p - X0 (components in x, y, z order whatever the axis), n = (ab.y ac.z - ab.z ac.y, ab.z ac.x - ab.x ac.z,
 *                           ab.x ac.y - ab.y ac.x), s = (n.x d.x + n.y d.y) + n.z d.z, hit = w > 0 ? s < 0 : s > 0.
 *                        4. A hit adds w to winding and 1 to crossings.
 *                      A ray through a shared edge or vertex is decided by the vertex classes and the canonical edge flags alone, which are
 *                      the same bits in every face that shares it: the count is that of the mesh's slice polygon, right for every query
 *                      that is not within rounding of the surface itself.
 *   the grid           n[2] cells (1 .. MOFA_WIND_MAX_GRID per axis) over (u, v) from origin[2] with cell[2] > 0 (HOST arrays of doubles).
 *                      idx(x) = t >= 0 ? (t < n ? (int) t : n - 1) : 0 with t = floor((x - origin) / cell); cell id = iu n[1] + iv.  A face
 *                      whose three u or whose three v have no extent (min == max) is FLAT: it enters no cell (it can never be crossed).
 *                      Every other face enters the cells idx(min u) .. idx(max u) x idx(min v) .. idx(max v).  A face can only count where
 *                      min u <= p.u < max u and min v <= p.v < max v and idx is monotone: the resolution changes no bit of the result.
 *   mofa_wind_bin_count    n_cells[f] (int64) = the cells face f enters; counts[MOFA_WIND_FLAT] += the flat faces
 *   mofa_wind_bin_emit     with offsets [F] (int64, DEVICE) = the exclusive sum of n_cells and P = its total (1 .. 2^31 - 1): pair_cell /
 *                          pair_face [P] (int32), face f's cells in ascending id from offsets[f].  The caller sorts the pairs stably by cell
 *                          (each cell's faces then ascend) and forms cell_start [cells + 1] (int32).
 *   mofa_wind_query        one thread per query; thread i takes query order[i] (int64 [N], DEVICE: a permutation that puts queries of one
 *                          cell next to each other; NULL = the identity), walks the faces pair_face[cell_start[c] .. cell_start[c + 1] - 1]
 *                          of the cell c of (idx(p.u), idx(p.v)) in list order and writes winding [N] and crossings [N] (int32).  A query
 *                          with a non-finite coordinate gets 0 / 0 and is counted in counts[MOFA_WIND_NON_FINITE].
 *                          counts[MOFA_WIND_TESTS] += the listed faces walked, counts[MOFA_WIND_MAX_COLUMN] = max(the longest list a query
 *                          walked): both depend on the grid, no result does.  P = 0 (0 .. 2^31 - 1): nothing is listed, cell_start is not
 *                          read and pair_face may be NULL.
 * A null pointer, an axis outside 0 .. 2 or a grid out of range returns MOFA_EINVAL with a message. */
enum { MOFA_WIND_NON_FINITE = 0, MOFA_WIND_FLAT = 1, MOFA_WIND_TESTS = 2, MOFA_WIND_MAX_COLUMN = 3, MOFA_WIND_COUNTS = 4 };
#define MOFA_WIND_MAX_GRID 4096
int mofa_wind_bin_count(const float* verts, const int32_t* faces, int64_t F, int64_t V, int32_t axis, const double origin[2], const double cell[2],
                        const int32_t n[2], int64_t* n_cells, int64_t* counts, void* stream);
int mofa_wind_bin_emit(const float* verts, const int32_t* faces, int64_t F, int64_t V, int32_t axis, const double origin[2], const double cell[2],
                       const int32_t n[2], const int64_t* offsets, int64_t P, int32_t* pair_cell, int32_t* pair_face, void* stream);
int mofa_wind_query(const float* points, int64_t N, const int64_t* order, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    int32_t axis, const double origin[2], const double cell[2], const int32_t n[2], const int32_t* cell_start,
                    const int32_t* pair_face, int64_t P, int32_t* winding, int32_t* crossings, int64_t* counts, void* stream);

/* Mesh ray casting: the first or the last hit of N rays o + t d on a triangle mesh (verts [V,3] float, faces [F,3] int32), through the grid
 * of face lists of the surface distance above (mofa_dist_bin_count / mofa_dist_bin_emit, the caller's sort, cell_start; mesh.py drives the
 * passes: mesh.ray_cast, mesh.ray_bounds; 1 <= N, V, F <= 2^31 - 1).  d is NOT normalised: t is the ray parameter.  No float or double
 * atomics: the same input gives the same bytes every time; the only atomics are the integer counters counts[MOFA_RAY_COUNTS] (int64,
 * DEVICE, zeroed by the caller; slot 0 is mofa_dist_bin_count's degenerate faces, so one buffer serves both).  The kernel checks the
 * indices it dereferences: a bad one is skipped.  It waits on no other thread and its loops are bounded by the grid's dimensions.  All
 * arithmetic is fp64 on the fp32 values widened, every operation rounded separately (no FMA).
 *   the pair           ray (o, d) against (a, b, c): the watertight test of Woop, Benthin and Wald (JCGT 2013)
 *                        kz = the axis of the largest |d| (a tie: the lowest axis), kx = (kz + 1) % 3, ky = (kz + 2) % 3, swapped when d[kz] < 0
 *                        Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]
 *                        for X = a, b, c:  X' = X - o;  Xx = X'[kx] - Sx X'[kz], Xy = X'[ky] - Sy X'[kz], Xz = Sz X'[kz]   (-> A, B, C)
 *                        U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax;  some of them < 0 and some > 0: a miss (zeros are inside)
 *                        det = (U + V) + W;  det == 0: a miss
 *                        t = ((U Az + V Bz) + W Cz) / det, then t = t < zlo ? zlo : t, t = t > zhi ? zhi : t with
 *                          zlo = Az < Bz ? Az : Bz, zlo = Cz < zlo ? Cz : zlo and zhi likewise with > (t is a convex combination of the three
 *                          depths: the clamp removes rounding only)
 *                        point[k] = o[k] + t d[k];  bary = (U / det, V / det, W / det);  front = det > 0 (the ray runs against (b - a) x (c - a))
 *                        the box rule:  tol = 2^-42 (((|o0| + |o1|) + |o2|) + ((m0 + m1) + m2)) with m[k] = max(|a[k]|, |b[k]|, |c[k]|);  the pair is
 *                          a miss (counts[MOFA_RAY_OFF_BOX]) when on some axis point[k] < min(a[k], b[k], c[k]) - tol or point[k] >
 *                          max(a[k], b[k], c[k]) + tol: the hit of a ray nearly in the face's plane, whose weights are rounding noise, counts
 *                          only where it lies on the face's own box.  A decision of the pair alone; the walk below leans on it.
 *                        accepted when t_min <= t <= t_max (both ends included) and cull does not exclude the side:
 *                          MOFA_RAY_CULL_BACK drops det < 0, MOFA_RAY_CULL_FRONT drops det > 0
 *                      The two products of an edge function are the same bits in both faces that share the edge and their differences exact
 *                      negatives: no ray passes between two faces.  MOFA_RAY_FIRST: the smaller t wins, MOFA_RAY_LAST: the larger, among equal
 *                      t the lower face index: the answer is a function of the mesh and the ray alone.
 *   mofa_ray_query     one thread per ray; thread i takes ray order[i] (int64 [N], DEVICE: a permutation that puts similar rays next to each
 *                      other; NULL = the identity) and writes its slots of t [N] (float), t64 [N] (double), face [N] (int32), front [N]
 *                      (uint8), bary [N,3] and point [N,3] (float, rounded once from fp64).  The grid (origin, cell, slack, n, cell ids, idx) is
 *                      the surface distance's.  With hi[k] = origin[k] + (double) n[k] cell[k], M[k] = max(|origin[k]|, |hi[k]|),
 *                      R = ((|o0| + |o1|) + |o2|) + ((M0 + M1) + M2), s[k] = slack[k] + 2^-40 R and Wt = |Sz| s[kz], the ray visits the slabs
 *                      j = 0 .. n[kz] - 1 of cells along kz in ray order (MOFA_RAY_LAST: in reverse); plane(j) = origin[kz] + (double) j cell[kz]:
 *                        Sz > 0:  lo_t = (plane(j) - o[kz]) Sz - Wt,      hi_t = (plane(j + 1) - o[kz]) Sz + Wt
 *                        Sz < 0:  lo_t = (plane(j + 1) - o[kz]) Sz - Wt,  hi_t = (plane(j) - o[kz]) Sz + Wt
 *                      Every hit of a face listed in slab j has lo_t <= t <= hi_t for one such j, and lo_t, hi_t are monotone
 *                      along the walk.  FIRST: the walk ends before slab j when (a hit is held and its t < lo_t, strictly: an equal t with a lower
 *                      index may sit there) or lo_t > t_max;  LAST: when (a hit is held and its t > hi_t) or hi_t < t_min.  With
 *                      ta = max(lo_t, t_min), tb = min(hi_t, t_max), a slab with not ta <= tb is passed over; in any other, for k = kx, ky:
 *                        pa = o[k] + ta d[k], pb = o[k] + tb d[k];  cells idx(min(pa, pb) - s[k]) .. idx(max(pa, pb) + s[k])
 *                      and every face listed in a cell of that rectangle of slab j is tested (a face tested twice changes nothing).
 *                      A ray with a non-finite origin or direction or with d = 0 gets face -1, t / t64 / bary / point NaN and is counted in
 *                      counts[MOFA_RAY_BAD]; a ray without a hit gets face -1, t and t64 +infinity, bary and point NaN.
 *                      counts[MOFA_RAY_TESTS] += the pairs tested, counts[MOFA_RAY_OFF_BOX] += those the box rule refused,
 *                      counts[MOFA_RAY_MAX_SLABS] = max(the slabs a ray visited): all three depend on the grid, no result bit does.
 *                      pair_face may be NULL when P = 0.
 * A null pointer, t_min > t_max or a NaN bound, an unknown which / cull or a grid out of range returns MOFA_EINVAL with a message. */
enum { MOFA_RAY_DEGENERATE = 0, MOFA_RAY_BAD = 1, MOFA_RAY_TESTS = 2, MOFA_RAY_MAX_SLABS = 3, MOFA_RAY_OFF_BOX = 4, MOFA_RAY_COUNTS = 5 };
enum { MOFA_RAY_FIRST = 0, MOFA_RAY_LAST = 1 };
enum { MOFA_RAY_CULL_NONE = 0, MOFA_RAY_CULL_BACK = 1, MOFA_RAY_CULL_FRONT = 2 };
int mofa_ray_query(const float* origins, const float* dirs, int64_t N, const int64_t* order, const float* verts, int64_t V,
                   const int32_t* faces, int64_t F, const double origin[3], const double cell[3], const double slack[3], const int32_t n[3],
                   const int32_t* cell_start, const int32_t* pair_face, int64_t P, double t_min, double t_max, int32_t which, int32_t cull,
                   float* t, double* t64, int32_t* face, uint8_t* front, float* bary, float* point, int64_t* counts, void* stream);

/* Depth-map fusion: a truncated signed distance volume (Curless and Levoy 1996; KinectFusion) with silhouette carving on the lattice of
 * mofa_grid_points (nx x ny x nz samples, idx = (i ny + j) nz + k, >= 2 samples per axis, nx ny nz < 2^31), integrated from depth frames
 * whose depth is the RAY PARAMETER of get_rays (what render_geometry without NDC, mofa_raster_resolve and mofa_ray_query return), and the
 * marchable field made from it: mofa_iso_count / mofa_iso_emit at level 0 give the surface the frames show (mesh.py drives the passes:
 * mesh.tsdf_volume / tsdf_integrate / tsdf_field / tsdf_surface).  One thread per voxel, no atomics: the same frames in the same order give
 * the same bytes, and the views [a | b] in two calls give the bytes of one call with a + b.  All arithmetic is fp64 on the fp32 inputs
 * widened, every operation rounded separately (no FMA).
 *   the state            per voxel acc (double: the weighted sum of the truncated distances), wsum (double: the sum of the weights), front
 *                        (int32: the observations that entered acc) and behind (int32: the views in which the voxel lay behind the seen
 *                        surface by more than trunc); four DEVICE arrays of nx ny nz elements, zeroed by the caller before the first frame.
 *                        mofa_tsdf_state_bytes = 24 nx ny nz, or 0 for a lattice that is refused.
 *   mofa_tsdf_integrate  depth [n_views,H,W] (float, DEVICE), weight the same shape or NULL (every weight 1; a weight must be finite and
 *                        >= 0: the CALLER checks), cams [n_cams,16] (float, DEVICE; n_cams = 1: one camera for every view, or n_views):
 *                        fx, fy, cx, cy, then the pose c[3][4] row-major (c2w of get_rays, ASSUMED orthonormal as in mofa_raster_project).
 *                        For the voxel at x (the bits of mofa_grid_points) and every view in order:
 *                          d[a] = x[a] - c[a][3];  p[a] = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a];  t = -p[2]
 *                          not t > 0: the view does not see the voxel
 *                          u = cx + fx (p0 / t), v = cy - fy (p1 / t);  pu = floor(u + 0.5), pv = floor(v + 0.5) (pixels are sampled at
 *                          integer points);  unless 0 <= pu < W and 0 <= pv < H (tested on the doubles: a non-finite value fails) the
 *                          view does not see the voxel
 *                          D = depth[view][pv][pu]:  not D > 0 (NaN, -infinity, 0, negative): unknown, skipped
 *                                                    D = +infinity: background; carve != 0: s = 1 (the ray's space is empty), else skipped
 *                                                    else sdf = D - t;  sdf < -trunc: behind += 1, skipped;  s = sdf / trunc, s > 1: s = 1
 *                          w = weight[view][pv][pu] or 1;  w == 0: skipped;  acc = acc + w s, wsum = wsum + w, front += 1
 *   mofa_tsdf_field      field [nx,ny,nz] (float): wsum > 0: (float)(-(acc / wsum)), positive inside; otherwise by `unobserved`:
 *                        MOFA_TSDF_UNOBSERVED_AUTO +1 if behind > 0 (only ever seen behind a surface) and -1 if never seen at all,
 *                        _OUTSIDE -1, _INSIDE +1.  close_border != 0 then sets the outermost lattice layer to -1.  The field is finite.
 *                        counts[MOFA_TSDF_COUNTS] (int64, DEVICE, written, not added to): the voxels with wsum > 0, those filled +1, those
 *                        filled -1 (the three classes partition the lattice, border or not) and the voxels of the outermost layer the
 *                        border overwrote (0 without close_border), by per-block sums in `workspace` (mofa_tsdf_workspace_bytes, DEVICE)
 *                        and one fixed-order pass over them.
 * A null pointer, a refused lattice, H or W < 1 or H W >= 2^31, n_views < 1, n_cams other than 1 or n_views, a trunc that is not finite and
 * positive or an unknown `unobserved` returns MOFA_EINVAL with a message. */
enum { MOFA_TSDF_OBSERVED = 0, MOFA_TSDF_FILLED_INSIDE = 1, MOFA_TSDF_FILLED_OUTSIDE = 2, MOFA_TSDF_BORDER = 3, MOFA_TSDF_COUNTS = 4 };
enum { MOFA_TSDF_UNOBSERVED_AUTO = 0, MOFA_TSDF_UNOBSERVED_OUTSIDE = 1, MOFA_TSDF_UNOBSERVED_INSIDE = 2 };
size_t mofa_tsdf_state_bytes(int64_t nx, int64_t ny, int64_t nz);
size_t mofa_tsdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int mofa_tsdf_integrate(int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], double trunc, const float* depth,
                        const float* weight, int64_t n_views, int32_t H, int32_t W, const float* cams, int64_t n_cams, int32_t carve, double* acc,
                        double* wsum, int32_t* front, int32_t* behind, void* stream);
int mofa_tsdf_field(int64_t nx, int64_t ny, int64_t nz, const double* acc, const double* wsum, const int32_t* behind, int32_t unobserved,
                    int32_t close_border, float* field, void* workspace, int64_t* counts, void* stream);

/* Multi-view colour baking: posed colour frames projected onto the vertices of a mesh with any triangulation (verts [V,3] float, 1 <= V <=
 * 2^31 - 1), occlusion-aware through one depth frame per view in the encoding of mofa_tsdf_integrate (the RAY PARAMETER of get_rays; +infinity
 * background; NaN, -infinity and values <= 0 unknown), and the vertex colours made from what was gathered (mesh.py drives the passes:
 * mesh.bake_state / bake_integrate / bake_colors / fill_colors).  One thread per vertex, no atomics: the same frames in the same order give the
 * same bytes, and the views [a | b] in two calls give the bytes of one call with a + b.  All arithmetic is fp64 on the fp32 inputs widened,
 * every operation rounded separately (no FMA).  1 <= C <= 16 channels.
 *   the state            per vertex csum [V,C] (double: the weighted colour sum), wsum [V] (double: the weight sum), wbest [V] (double: the
 *                        largest weight so far), cbest [V,C] (float: the colour of the view with the largest weight so far), seen [V] (int32:
 *                        the views that entered), occluded [V] (int32: the views in which the vertex failed the depth test) and grazing [V]
 *                        (int32: the views the angle test rejected); seven DEVICE arrays, zeroed by the caller before the first frame.
 *   mofa_bake_integrate  normals [V,3] (float, DEVICE) or NULL, images [n_views,H,W,C] and depth [n_views,H,W] (float, DEVICE), cams
 *                        [n_cams,16] exactly as mofa_tsdf_integrate (n_cams = 1 or n_views).  For the vertex x and every view in order:
 *                          d[a] = x[a] - c[a][3];  p[a] = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a];  t = -p[2];  not t > 0: skipped
 *                          u = cx + fx (p0 / t), v = cy - fy (p1 / t);  u0 = floor(u), v0 = floor(v);  unless 0 <= u0, u0 + 1 <= W - 1,
 *                          0 <= v0 and v0 + 1 <= H - 1 (tested on the doubles: a non-finite value fails; only then are integer offsets
 *                          formed, so every load is in bounds): skipped
 *                          D_k = depth[view] at (v0, u0), (v0, u0 + 1), (v0 + 1, u0), (v0 + 1, u0 + 1):  any D_k unknown or background:
 *                          skipped (the silhouette erodes);  any t - D_k > depth_tol: occluded += 1, skipped (so do occlusion boundaries)
 *                          with normals n:  e = -d;  cosv = ((n0 e0 + n1 e1) + n2 e2) / sqrt((e0 e0 + e1 e1) + e2 e2);  not cosv > cos_min:
 *                          grazing += 1, skipped;  w = 1.0, then `power` times w = w cosv (no pow);  without normals w = 1
 *                          fu = u - u0, fv = v - v0;  per channel, with c00, c10, c01, c11 the texels at the four corners in the order
 *                          above:  a = c00 + fu (c10 - c00), b = c01 + fu (c11 - c01), col = a + fv (b - a);  any of the 4 C texels not
 *                          finite: skipped
 *                          csum = csum + w col, wsum = wsum + w, seen += 1;  w > wbest (strict: the earlier view keeps a tie): wbest = w,
 *                          cbest = (float)col
 *   mofa_bake_resolve    colors [V,C] (float) and valid [V] (uint8): blend MOFA_BAKE_MEAN: (float)(csum / wsum) where wsum > 0;
 *                        MOFA_BAKE_BEST: cbest where seen > 0; everywhere else `fill` and valid = 0.  counts[MOFA_BAKE_COUNTS] (int64,
 *                        DEVICE, written, not added to): the coloured vertices, the uncoloured ones with occluded > 0, the uncoloured ones
 *                        with grazing > 0 only, and the uncoloured ones no view held in a footprint with a known surface (the four classes
 *                        partition the vertices), by per-block sums in `workspace` (DEVICE, 16 ((V + 255) / 256) bytes) and one
 *                        fixed-order pass over them.
 *   mofa_bake_fill       one Jacobi step of hole filling over mesh.vertex_adjacency's lists (offsets [V + 1] int64, nbr [E] int32, 0 <= E
 *                        <= 2^31 - 1), double-buffered (input and output must differ): an invalid vertex with k >= 1 valid neighbours takes
 *                        (float)(s / k) per channel, s = 0.0 then s = s + (double)colors_in[j] over its valid neighbours j in list order,
 *                        and valid_out = 1; every other vertex is copied.  A list that leaves [0, E) or a neighbour outside [0, V) is not
 *                        dereferenced.
 * A null pointer, V or C out of range, H or W < 2 or H W >= 2^31, n_views < 1, n_cams other than 1 or n_views, a depth_tol that is not finite
 * and >= 0, cos_min outside [0, 1), power outside 0 .. 8 or an unknown blend returns MOFA_EINVAL with a message. */
enum { MOFA_BAKE_COLORED = 0, MOFA_BAKE_OCCLUDED = 1, MOFA_BAKE_GRAZING = 2, MOFA_BAKE_UNSEEN = 3, MOFA_BAKE_COUNTS = 4 };
enum { MOFA_BAKE_MEAN = 0, MOFA_BAKE_BEST = 1 };
int mofa_bake_integrate(const float* verts, const float* normals, int64_t V, const float* images, const float* depth, int64_t n_views, int32_t H,
                        int32_t W, int32_t C, const float* cams, int64_t n_cams, double depth_tol, double cos_min, int32_t power, double* csum,
                        double* wsum, double* wbest, float* cbest, int32_t* seen, int32_t* occluded, int32_t* grazing, void* stream);
int mofa_bake_resolve(int64_t V, int32_t C, const double* csum, const double* wsum, const float* cbest, const int32_t* seen,
                      const int32_t* occluded, const int32_t* grazing, int32_t blend, float fill, float* colors, uint8_t* valid, void* workspace,
                      int64_t* counts, void* stream);
int mofa_bake_fill(const float* colors_in, const uint8_t* valid_in, int64_t V, int32_t C, const int64_t* offsets, const int32_t* nbr, int64_t E,
                   float* colors_out, uint8_t* valid_out, void* stream);

/* UV texture baking: the map between the texels of a texture image and the surface of a mesh with an OBJ-style per-corner UV layout (uvs
 * [T,2] float, uv_faces [F,3] int32: uv_faces[f][k] is the UV of corner k of faces[f]; T != V and seams are normal), and the image-side
 * operations around mofa_bake_integrate, which takes the texels' surface points as it takes vertices (mesh.py drives the passes:
 * mesh.uv_locate / texel_map / texel_surface / texture_image / dilate_texture / sample_texture).  A texture is [Ht,Wt,C] float, row 0 at
 * the top, 1 <= C <= 16, Ht Wt < 2^31: texel (i, j) has its centre at u = (j + 0.5) / Wt, v = 1 - (i + 0.5) / Ht, and a UV maps to the
 * continuous texel coordinates x = u Wt - 0.5, y = (1 - v) Ht - 0.5; no wrap-around; UVs outside [0, 1] are legal and see no texel.  One
 * thread per element; all arithmetic is fp64 on the fp32 inputs widened, every operation rounded separately (no FMA); no float or double
 * atomics: the same input gives the same bytes every time; the only atomics are the integer counters (int64, DEVICE, zeroed by the caller,
 * one atomic per wavefront).  Every kernel checks the indices it dereferences: a bad one is skipped and counted.  1 <= N, T, V, F <= 2^31 - 1.
 *   mofa_uv_locate   for queries [N,2] (double, DEVICE) the UV triangle that holds each: face [N] (int32, -1: none) and bary [N,3] (double,
 *                    NaN where none).  The faces are listed per cell of a 2-D grid over (u, v) by mofa_wind_bin_count / _emit on the UVs as
 *                    a zero-padded [T,3] copy with axis = 2 (every cell a face's closed UV box touches; the faces they drop as flat have no
 *                    UV area), sorted stably by cell into cell_start [cells + 1] / pair_face [P] exactly as for mofa_wind_query, with the
 *                    same origin / cell / n and the same permutation `order` (NULL = the identity).  A query walks the list of the cell
 *                    of (idx(q.u), idx(q.v)).  Against face f with UV corners A, B, C:
 *                      D = (B.u - A.u) (C.v - A.v) - (B.v - A.v) (C.u - A.u);  D == 0 or not finite: the face is skipped
 *                      edge k is the one opposite corner k (B -> C, C -> A, A -> B); of its endpoints P is the lexicographically smaller
 *                      (u, then v) and Q the other:  E = (Q.u - P.u) (q.v - P.v) - (Q.v - P.v) (q.u - P.u), negated where the face runs
 *                      the edge from Q to P, and negated again when D < 0 (a mirrored chart): e_k.  Two faces that share an edge - by
 *                      index or, across a seam, by equal coordinates - compute the same bits up to an exact sign.
 *                      inside: e_0 >= 0, e_1 >= 0, e_2 >= 0 (zeros count, so a point on a shared edge cannot fall between two faces) and
 *                      S = (e_0 + e_1) + e_2 > 0;  bary_k = e_k / S;  among the containing faces the lowest index wins.
 *                    counts[MOFA_UV_DEGENERATE] += the faces of the layout whose D is 0 or not finite, [MOFA_UV_NON_FINITE] += the queries
 *                    with a non-finite coordinate (face -1), [MOFA_UV_MULTI] += the queries STRICTLY inside (all e_k > 0) two or more
 *                    faces (overlapping charts), [MOFA_UV_TESTS] += the listed faces walked (depends on the grid; no result does: a face
 *                    can hold q only where its box does, and idx is monotone).  P = 0: nothing is listed, pair_face may be NULL.
 *   mofa_uv_surface  per element (face [N] int32, bary [N,3] double) a surface point and a unit normal (float [N,3] each): with X_k =
 *                    verts[faces[f][k]],  point[a] = (float)((b0 X0[a] + b1 X1[a]) + b2 X2[a]);  with normals [V,3] (float, DEVICE) m =
 *                    the same interpolation of the vertex normals, with NULL m = (X1 - X0) x (X2 - X0) (p = X1 - X0, r = X2 - X0: p.y r.z
 *                    - p.z r.y, p.z r.x - p.x r.z, p.x r.y - p.y r.x; it follows the faces' winding);  len = sqrt((m.x m.x + m.y m.y) +
 *                    m.z m.z);  normal = (float)(m / len), (0, 0, 0) unless len > 0 and finite.  A face outside [0, F) or a vertex index
 *                    outside [0, V): point NaN, normal 0, counts[0] += 1.
 *   mofa_uv_dilate   one gutter-filling step on the image grid, double-buffered (input and output must differ): an invalid texel with k >=
 *                    1 valid texels among its 8 neighbours inside the image takes (float)(s / k) per channel, s = 0.0 then s = s +
 *                    (double)texture_in[neighbour] over the valid ones in row-major order of the 3 x 3 window, and valid_out = 1; every
 *                    other texel is copied (a baked texel never changes).  valid: uint8 [Ht,Wt].
 *   mofa_uv_sample   the texture lookup of a rasterised view: per pixel face [N] (int32) and bary [N,3] (float), as mofa_raster_resolve
 *                    writes them:  u = (b0 u0 + b1 u1) + b2 u2 over the corners' UVs, v likewise (doubles, never rounded to float);  x, y
 *                    as above;  j0 = floor(x), fx = x - j0, i0 = floor(y), fy = y - i0;  the indices j0, j0 + 1, i0, i0 + 1 clamped to
 *                    the image;  per channel a = c00 + fx (c10 - c00), b = c01 + fx (c11 - c01), out = (float)(a + fy (b - a)), c10 the
 *                    texel (i0, j0 + 1) (mofa_bake_integrate's order).  face outside [0, F) (-1: nothing was hit), a UV index outside [0,
 *                    T) or a non-finite u or v: `background`, counts[0] += 1.
 * A null pointer, a count or an image size out of range, C outside 1 .. 16 or a grid out of range returns MOFA_EINVAL with a message. */
enum { MOFA_UV_DEGENERATE = 0, MOFA_UV_NON_FINITE = 1, MOFA_UV_TESTS = 2, MOFA_UV_MULTI = 3, MOFA_UV_COUNTS = 4 };
int mofa_uv_locate(const double* queries, int64_t N, const int64_t* order, const float* uvs, int64_t T, const int32_t* uv_faces, int64_t F,
                   const double origin[2], const double cell[2], const int32_t n[2], const int32_t* cell_start, const int32_t* pair_face, int64_t P,
                   int32_t* face, double* bary, int64_t* counts, void* stream);
int mofa_uv_surface(const int32_t* face, const double* bary, int64_t N, const float* verts, int64_t V, const int32_t* faces, int64_t F,
                    const float* normals, float* points, float* normals_out, int64_t* counts, void* stream);
int mofa_uv_dilate(const float* texture_in, const uint8_t* valid_in, int32_t Ht, int32_t Wt, int32_t C, float* texture_out, uint8_t* valid_out,
                   void* stream);
int mofa_uv_sample(const int32_t* face, const float* bary, int64_t N, const float* uvs, int64_t T, const int32_t* uv_faces, int64_t F,
                   const float* texture, int32_t Ht, int32_t Wt, int32_t C, float background, float* out, int64_t* counts, void* stream);

/* Mesh smoothing: Taubin lambda | mu filtering of the vertices of a triangle mesh (verts [V,3] float, faces [F,3] int32) over a fixed-order
 * vertex adjacency (mesh.py drives the passes: mesh.vertex_adjacency, mesh.smooth; 1 <= V, F, E <= 2^31 - 1).  No float or double atomics and
 * a fixed summation order: the same input gives the same bytes every time; the only atomics are the integer counters
 * counts[MOFA_SMOOTH_COUNTS] (int64, DEVICE, zeroed by the caller).  Every kernel checks the indices it dereferences: a bad one is counted in
 * counts[MOFA_SMOOTH_BAD_INDEX] and skipped.  No kernel waits on another thread.  All arithmetic is fp64 on the fp32 coordinates widened,
 * every operation rounded separately (no FMA).
 *   the adjacency      half-edge entry e = 2 (3 f + c) + dir, c = 0 .. 2, carries the directed pair (a, b) for dir = 0 and (b, a) for dir = 1
 *                      with a = faces[f][(c + 1) % 3], b = faces[f][(c + 2) % 3] (the edge opposite corner c).  The caller drops the entries
 *                      with a == b, sorts the rest stably by the key (i << 31) | j — perm [P] (int64) holds the sorted entries' e, ascending
 *                      inside a run of equal keys — and forms seg [E + 1] (int64), the run boundaries of the E distinct pairs; nbr [E]
 *                      (int32) = j of every pair and offsets [V + 1] (int64) = the first pair of every i.
 *   mofa_smooth_corner_cots   cots [F,3] (double): for corner c of face f with apex o = faces[f][c] and a, b as above,
 *                               u = x_a - x_o, v = x_b - x_o;  cr = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx);
 *                               n = sqrt((crx crx + cry cry) + crz crz);  cots[3 f + c] = ((ux vx + uy vy) + uz vz) / n
 *                             n == 0 or not finite: cots = 0 and counts[MOFA_SMOOTH_FLAT_CORNERS] += 1.
 *   mofa_smooth_edge_weights  weights [E] (double), one thread per pair p:  w = 0.0;  for k = seg[p] .. seg[p + 1] - 1 in that order:
 *                             w += 0.5 * cots[perm[k] / 2];  then w < 0: w = 0 and counts[MOFA_SMOOTH_NEGATIVE_WEIGHTS] += 1.  The runs of
 *                             (i, j) and (j, i) hold the same corners in the same order: w_ij == w_ji bit for bit.  F is that of cots.
 *   mofa_smooth_step          one thread per vertex i, its neighbours j = nbr[k], k = offsets[i] .. offsets[i + 1] - 1, in that order, per
 *                             component x:
 *                               weights == NULL:  s = 0.0;  s += (double)x_j - (double)x_i;  L = s / (double)(offsets[i + 1] - offsets[i])
 *                               weights [E]:      s = 0.0, sw = 0.0;  s += weights[k] * ((double)x_j - (double)x_i), sw += weights[k];
 *                                                 sw > 0: L = s / sw; otherwise the vertex keeps its bits, counts[MOFA_SMOOTH_ZERO_WEIGHT] += 1
 *                               verts_out = (float)((double)x_i + factor * L)
 *                             A vertex with pinned[i] != 0 (uint8 [V]; NULL: none) or without neighbours keeps its bits.  A vertex with a
 *                             neighbour outside [0, V) or a list outside [0, E) writes nothing and is counted.  verts_in != verts_out: the
 *                             step never runs in place; the caller alternates two buffers. */
enum { MOFA_SMOOTH_FLAT_CORNERS = 0, MOFA_SMOOTH_NEGATIVE_WEIGHTS = 1, MOFA_SMOOTH_ZERO_WEIGHT = 2, MOFA_SMOOTH_BAD_INDEX = 3,
       MOFA_SMOOTH_COUNTS = 4 };
int mofa_smooth_corner_cots(const float* verts, const int32_t* faces, int64_t F, int64_t V, double* cots, int64_t* counts, void* stream);
int mofa_smooth_edge_weights(const double* cots, int64_t F, const int64_t* perm, int64_t P, const int64_t* seg, int64_t E, double* weights,
                             int64_t* counts, void* stream);
int mofa_smooth_step(const float* verts_in, int64_t V, const int64_t* offsets, const int32_t* nbr, int64_t E, const double* weights,
                     const uint8_t* pinned, double factor, float* verts_out, int64_t* counts, void* stream);

/* Mesh registration: the estimation step of rigid / similarity ICP (mesh.py drives the loop: mesh.register, mesh.fit_transform; the
 * correspondences come from mofa_dist_query; 1 <= N, V, F <= 2^31 - 1).  No atomics of any kind and a fixed summation order that does not
 * depend on the launch geometry: the same input gives the same bytes every time.  Every kernel checks the indices it dereferences; a
 * correspondence with a bad one counts as rejected.  No kernel waits on another thread.  All arithmetic is fp64 on the fp32 inputs widened,
 * every operation rounded separately (no FMA).
 *   mofa_icp_apply    transform = [s, R (row-major 3 x 3), t] (13 doubles, HOST);  out [N,3] (float):
 *                       out[i][r] = (float)(s * ((R[r][0] * x0 + R[r][1] * x1) + R[r][2] * x2) + t[r])
 *   mofa_icp_terms    terms [N,36] (double).  Correspondence i has the moved point y = moved[i], the target point c = target[i], the weight
 *                     w = weight[i] (double) and, for the plane metric, the unit normal n: with `face` ([N] int32; normals NULL) the normal of
 *                     the closest face, ab = b - a, ac = c - a of faces[face[i]] on verts,
 *                       cr = (ab_y ac_z - ab_z ac_y, ab_z ac_x - ab_x ac_z, ab_x ac_y - ab_y ac_x);  n = cr / sqrt((cr_x cr_x + cr_y cr_y) + cr_z cr_z)
 *                     and with `normals` ([N,3] float; face NULL) that row, as it is.  With yh = y - pivot and d = y - c, the unknowns
 *                     x = (omega_1..3, tau_1..3, sigma) — a small rotation about the pivot, a translation, a relative scale — see the rows
 *                       MOFA_ICP_POINT:  J0 = [0, yh_z, -yh_y, 1, 0, 0, yh_x],  J1 = [-yh_z, 0, yh_x, 0, 1, 0, yh_y],
 *                                        J2 = [yh_y, -yh_x, 0, 0, 0, 1, yh_z]  (that is [-[yh]x | I | yh]),  r = d
 *                                        A_ab = w * ((J0a * J0b + J1a * J1b) + J2a * J2b),  g_a = w * ((J0a * r0 + J1a * r1) + J2a * r2),
 *                                        e = w * ((r0 * r0 + r1 * r1) + r2 * r2)
 *                       MOFA_ICP_PLANE:  J = [yh_y n_z - yh_z n_y, yh_z n_x - yh_x n_z, yh_x n_y - yh_y n_x, n_x, n_y, n_z,
 *                                             (n_x * yh_x + n_y * yh_y) + n_z * yh_z]  (that is [yh x n | n | n . yh]),
 *                                        r = (n_x * d_x + n_y * d_y) + n_z * d_z;  A_ab = w * (Ja * Jb),  g_a = w * (Ja * r),  e = w * (r * r)
 *                     terms[i] = A's upper triangle row by row (A_00 .. A_06, A_11 .. A_66: 28 numbers), g_0 .. g_6, e.  A correspondence
 *                     is rejected — 36 exact +0.0 — when `w > 0` is false, or a face / vertex index lies outside the mesh.  The step solves
 *                     (sum A) x = -(sum g).  The point metric ignores face / normals / the mesh.
 *   mofa_icp_reduce   out [ceil(M / MOFA_ICP_CHUNK), ncols] (double) from in [M, ncols], 1 <= ncols <= 36: chunk k holds the rows
 *                     [1024 k, min(1024 (k + 1), M)); thread t of its 256 starts at 0.0 and adds the chunk's rows t, t + 256, t + 512,
 *                     t + 768 (those below M) in that order; then `for w = 128, 64, .. 1: p[t] += p[t + w] for t < w` over the 256 partial
 *                     sums, and p[0] is the chunk's row.  The caller reduces the chunk rows the same way until one row is left.  in != out.
 *   mofa_icp_terms_reduce   partial [ceil(N / MOFA_ICP_CHUNK), 36]: mofa_icp_reduce of mofa_icp_terms' matrix without that matrix reaching
 *                     memory — the same additions in the same order (a rejected row adds its zeros), the same bits.
 *   mofa_icp_reject   rejected [N] (uint8): the border rule on what mofa_dist_query returned.  face_border [F] (uint8): bit k set when the
 *                     edge opposite corner k of the face is a border edge (one use over both directions); vert_border [V] (uint8): the
 *                     vertex lies on a border edge.  With z_k = (bary[i][k] == 0.0f), exactly, f = face[i]:
 *                       rejected = any k: z_k and bit k of face_border[f];  or two of the z_k hold and vert_border[faces[f][the third k]]
 *                     face[i] outside [0, F): 0 (no correspondence: the caller's rule, not this one).
 * A null pointer, a count out of range, an unknown metric, a non-finite pivot, or the plane metric with both or neither of face / normals
 * returns MOFA_EINVAL with a message. */
#define MOFA_ICP_TERMS 36
#define MOFA_ICP_CHUNK 1024
enum { MOFA_ICP_POINT = 0, MOFA_ICP_PLANE = 1 };
int mofa_icp_apply(const float* points, int64_t N, const double transform[13], float* out, void* stream);
int mofa_icp_terms(const float* moved, const float* target, const float* normals, const int32_t* face, const float* verts, int64_t V,
                   const int32_t* faces, int64_t F, const double* weight, int64_t N, const double pivot[3], int32_t metric, double* terms,
                   void* stream);
int mofa_icp_terms_reduce(const float* moved, const float* target, const float* normals, const int32_t* face, const float* verts, int64_t V,
                          const int32_t* faces, int64_t F, const double* weight, int64_t N, const double pivot[3], int32_t metric,
                          double* partial, void* stream);
int mofa_icp_reduce(const double* in, int64_t M, int32_t ncols, double* out, void* stream);
int mofa_icp_reject(const int32_t* face, const float* bary, int64_t N, const int32_t* faces, int64_t F, int64_t V, const uint8_t* face_border,
                    const uint8_t* vert_border, uint8_t* rejected, void* stream);

/* Non-rigid mesh registration: the linear step of stiffness-regularised ICP with one translation per template vertex (mesh.py drives the
 * loop: mesh.warp, mesh.warp_to; the correspondences come from mofa_dist_query, the border rule from mofa_icp_reject, the adjacency is
 * mofa_smooth_step's: offsets [V + 1] (int64), nbr [E] (int32); 1 <= V <= 2^31 - 1, 0 <= E <= 2^31 - 1).  The template is verts v [V,3]
 * (float), the unknown a displacement d [V,3] (double).  One step minimises
 *     sum_i w_i rho_i(v_i + d_i - c_i)  +  alpha sum_{edges {i,j}} |d_i - d_j|^2  +  sum_i h_i |v_i + d_i - p_i|^2
 * whose normal equations are (D + alpha L (x) I3) d = b, D_i a symmetric 3 x 3 block per vertex, L_ii = deg_i, L_ij = -1 for neighbours.
 * No atomics of any kind and a fixed summation order that does not depend on the launch geometry: the same input gives the same bytes every
 * time.  No kernel waits on another thread or workgroup.  Every kernel checks the indices it dereferences.  All arithmetic is fp64 (fp32
 * inputs widened first), every operation rounded separately (no FMA).
 *   mofa_warp_apply   out [V,3] (float):  out[i][k] = (float)((double)verts[i][k] + disp[i][k])
 *   mofa_warp_system  one thread per vertex i: v = verts[i], y = moved[i], c = target[i], w = weight[i] (double); for the plane metric the unit
 *                     normal n exactly as mofa_icp_terms takes it (`face` [V] on the target mesh tverts / tfaces, or `normals` [V,3]).
 *                       u_k = (double)c_k - (double)v_k;   r_k = (double)y_k - (double)c_k;   rr = (r_0 r_0 + r_1 r_1) + r_2 r_2
 *                       MOFA_ICP_POINT:  D_kk = w, D_kl = 0;  b_k = w * u_k;  e = w * rr
 *                       MOFA_ICP_PLANE:  D_kk = w * (n_k * n_k + point_weight),  D_kl = w * (n_k * n_l)  (k < l);
 *                                        nu = (n_0 u_0 + n_1 u_1) + n_2 u_2;   b_k = w * (n_k * nu + point_weight * u_k);
 *                                        nr = (n_0 r_0 + n_1 r_1) + n_2 r_2;   e = w * (nr * nr + point_weight * rr)
 *                     The data term is rejected — D, b, e exact +0.0 — when `w > 0` is false or (plane, by face) the face or one of its
 *                     vertices lies outside the target mesh.  Then, with handle_weight [V] (double; NULL: none) and h = handle_weight[i] > 0:
 *                       D_kk += h;   b_k += h * ((double)handle_pos[i][k] - (double)v_k)
 *                     and with deg = offsets[i + 1] - offsets[i]:   m_k = D_kk + alpha * (double)deg;   minv_k = m_k > 0 ? 1.0 / m_k : 0.0.
 *                     Outputs: D [V,6] (xx, xy, xz, yy, yz, zz), b [V,3], minv [V,3], energy [V] (e), all double.  A vertex whose list does
 *                     not lie in [0, E) gets deg = 0 and minv = 0 and is counted: bad [ceil(V / 256)] (int64) holds the count of each
 *                     workgroup of 256 vertices (written, not added to).
 *   mofa_warp_matvec  q = (D + alpha L (x) I3) p, one thread per vertex i over nbr[offsets[i] .. offsets[i + 1]) in that order:
 *                       s_k = 0.0;  s_k += p[j][k];   deg = (double)(offsets[i + 1] - offsets[i])
 *                       q_0 = ((D_xx p_0 + D_xy p_1) + D_xz p_2) + alpha * (deg * p_0 - s_0)
 *                       q_1 = ((D_xy p_0 + D_yy p_1) + D_yz p_2) + alpha * (deg * p_1 - s_1)
 *                       q_2 = ((D_xz p_0 + D_yz p_1) + D_zz p_2) + alpha * (deg * p_2 - s_2)
 *                     and partial [ceil(V / MOFA_ICP_CHUNK)] = the first level of p . q (mofa_warp_dot's, fused).  A vertex with a list outside
 *                     [0, E) or a neighbour outside [0, V) writes nothing, adds nothing to the sum and is counted: bad [ceil(V /
 *                     MOFA_ICP_CHUNK)] (int64) holds the count of each chunk (written).  p != q.
 *   mofa_warp_dot     partial [ceil(V / MOFA_ICP_CHUNK)] (double): the first level of the sum of term_i = (a_0 b_0 + a_1 b_1) + a_2 b_2 over
 *                     the rows of a, b [V,3] (double), exactly as mofa_icp_reduce sums a one-column matrix of the terms; the caller
 *                     reduces the partial sums with mofa_icp_reduce (ncols = 1) until one number is left.
 *   mofa_warp_solve   Jacobi-preconditioned conjugate gradients on A = D + alpha L (x) I3 from the start x [V,3] (double, in and out):
 *                       q = A x;  r = b - q;  z = minv * r (per component);  p = z;  rho_0 = r . z
 *                       step s = 0 .. K - 1:   q = A p;  pq = p . q;  [scalar]  a = rho_s / pq;
 *                                              x += a * p;  r = r - a * q;  z = minv * r;  rho_{s+1} = r . z;  p = z + (rho_{s+1} / rho_s) * p
 *                     every inner product by mofa_warp_dot's sum, its first level fused into the kernel that writes the vectors.  [scalar] is
 *                     one thread: the solve FREEZES at step s when rho_s <= cg_tol^2 * rho_0 (MOFA_WARP_STOP_TOLERANCE), else when
 *                     `pq > 0` is false (MOFA_WARP_STOP_BREAKDOWN).  The flag lives in device memory and is sticky: from then on no step
 *                     writes x, r, z, p or q, so every vector keeps its bits, and rho_{s+1} = rho_s.  The K steps are enqueued without a
 *                     host read or a synchronisation.  rec [MOFA_WARP_REC_RHO + K + 1] (double, DEVICE; cleared by the solve):
 *                     rec[MOFA_WARP_REC_A] the last a (0 once frozen), _FROZEN 0 / 1, _CAUSE 0 or MOFA_WARP_STOP_*, _STEPS the steps that
 *                     moved x, _TOL2 = cg_tol * cg_tol, rec[MOFA_WARP_REC_RHO + s] = rho_s for s = 0 .. K.  work holds
 *                     mofa_warp_workspace_doubles(V) doubles (r, z, p, q and the levels of the two sums); bad as mofa_warp_matvec's.
 *                     1 <= cg_iterations <= MOFA_WARP_MAX_CG, 0 <= cg_tol < 1.
 * As-rigid-as-possible stiffness (mesh.warp(stiffness_model = "arap"), mesh.deform): the stiffness term becomes
 *     alpha / 2 sum_i sum_{j in N(i)} |(y_i - y_j) - R_i (v_i - v_j)|^2,   y = v + d,   R_i a rotation per vertex,
 * whose normal equations in d keep the matrix D + alpha L (x) I3 and add alpha g to b.  Both kernels run one thread per vertex i over
 * nbr[offsets[i] .. offsets[i + 1]) in that order, with v widened to double:  e = v_i - v_j  (per component).
 *   mofa_warp_rotations  the rotation R [V,9] (double, row-major) that maximises sum_j e' . R e,  e'_c = e_c + (d_i,c - d_j,c), by Horn's
 *                     quaternion form:
 *                       S_ab = 0.0;  S_ab += e_a * e'_b   (a, b = x, y, z: nine sums)
 *                       N_00 = (Sxx + Syy) + Szz;  N_01 = Syz - Szy;  N_02 = Szx - Sxz;  N_03 = Sxy - Syx;
 *                       N_11 = (Sxx - Syy) - Szz;  N_12 = Sxy + Syx;  N_13 = Szx + Sxz;
 *                       N_22 = (Syy - Sxx) - Szz;  N_23 = Syz + Szy;  N_33 = (Szz - Sxx) - Syy;   N symmetric,  W = I (4 x 4)
 *                     then MOFA_WARP_JACOBI_SWEEPS sweeps over the pairs (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair with
 *                     N_pq == 0 is skipped, otherwise with x = N_pq:
 *                       theta = (N_qq - N_pp) / (2.0 * x);   t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
 *                       c = 1.0 / sqrt(t * t + 1.0);   s = t * c;
 *                       N_pp = N_pp - t * x;   N_qq = N_qq + t * x;   N_pq = N_qp = 0.0;
 *                       k != p, q:      N_kp' = c * N_kp - s * N_kq;   N_kq' = s * N_kp + c * N_kq   (both from the old values; N stays symmetric)
 *                       k = 0 .. 3:     W_kp' = c * W_kp - s * W_kq;   W_kq' = s * W_kp + c * W_kq
 *                     Afterwards m = the index of the largest N_mm, the lowest among equal ones (0, then 1, 2, 3 each only when strictly
 *                     larger), q = column m of W, n = sqrt(((q_0 q_0 + q_1 q_1) + q_2 q_2) + q_3 q_3), (w, x, y, z) = q / n and
 *                       R = [1 - 2 (yy + zz),  2 (xy - wz),  2 (xz + wy);   2 (xy + wz),  1 - 2 (xx + zz),  2 (yz - wx);
 *                            2 (xz - wy),  2 (yz + wx),  1 - 2 (xx + yy)]     (products first, e.g. 1.0 - 2.0 * (y * y + z * z))
 *                     and fit [V] (double):  fit = 0.0;  r_c = e'_c - ((R_c0 e_0 + R_c1 e_1) + R_c2 e_2);  fit += (r_0 r_0 + r_1 r_1) + r_2 r_2.
 *                     Always a proper rotation, also for a flat (rank 2) neighbourhood; with d = 0, S is symmetric, row 0 of N is never
 *                     rotated and R is the identity bit for bit (an empty list: S = 0, the identity).  A non-finite entry of S or of R
 *                     gives R = I, fit = 0 and is counted; a list outside [0, E) or a neighbour outside [0, V) gives R = I, fit = 0 and
 *                     is counted apart: bad [ceil(V / 256)][2] (int64; written): per workgroup of 256 vertices the index faults, then
 *                     the non-finite fits.  No NaN leaves the kernel.
 *   mofa_warp_arap_rhs   b [V,3] (double, in and out):  g_c = 0.0;  Rs = R_i + R_j (entrywise);  t_c = (Rs_c0 e_0 + Rs_c1 e_1) + Rs_c2 e_2;
 *                     g_c += 0.5 * t_c - e_c;  then  b_c = b_c + alpha * g_c.  All R = I gives g = 0 exactly.  A vertex with a bad list
 *                     or neighbour leaves its b alone and is counted: bad [ceil(V / 256)] (int64; written).  R != b.
 * A null pointer, a count out of range, an unknown metric, a negative or non-finite alpha / point_weight, the plane metric with both or
 * neither of face / normals, or handle weights without positions returns MOFA_EINVAL with a message. */
#define MOFA_WARP_MAX_CG 10000
enum { MOFA_WARP_REC_A = 0, MOFA_WARP_REC_FROZEN = 1, MOFA_WARP_REC_CAUSE = 2, MOFA_WARP_REC_STEPS = 3, MOFA_WARP_REC_TOL2 = 4,
       MOFA_WARP_REC_RHO = 8 };
enum { MOFA_WARP_STOP_TOLERANCE = 1, MOFA_WARP_STOP_BREAKDOWN = 2 };
int mofa_warp_apply(const float* verts, const double* disp, int64_t V, float* out, void* stream);
int mofa_warp_system(const float* verts, const float* moved, const float* target, const float* normals, const int32_t* face, const float* tverts,
                     int64_t TV, const int32_t* tfaces, int64_t TF, const double* weight, const double* handle_weight, const float* handle_pos,
                     const int64_t* offsets, int64_t E, int64_t V, int32_t metric, double point_weight, double alpha, double* D, double* b,
                     double* minv, double* energy, int64_t* bad, void* stream);
int mofa_warp_matvec(const double* D, const double* p, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double alpha, double* q,
                     double* partial, int64_t* bad, void* stream);
int mofa_warp_dot(const double* a, const double* b, int64_t V, double* partial, void* stream);
size_t mofa_warp_workspace_doubles(int64_t V);
int mofa_warp_solve(const double* D, const double* b, const double* minv, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V,
                    double alpha, int32_t cg_iterations, double cg_tol, double* x, double* work, double* rec, int64_t* bad, void* stream);
#define MOFA_WARP_JACOBI_SWEEPS 7 /* 5 bring the off-diagonal norm of N below 2^-50 of its norm on the tests' catalogue; + 2 */
int mofa_warp_rotations(const float* verts, const double* disp, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double* R,
                        double* fit, int64_t* bad, void* stream);
int mofa_warp_arap_rhs(const float* verts, const double* R, const int64_t* offsets, const int32_t* nbr, int64_t E, int64_t V, double alpha,
                       double* b, int64_t* bad, void* stream);

/* Linear shape models: the device side of mesh.shape_model / shape_synthesize / shape_project / shape_fit (mesh.py drives them; the
 * M x M eigen-decomposition and the K x K solves run on the host).  No atomics of any kind and a fixed summation order that does not depend
 * on the launch geometry or on how the pairs are tiled: the same input gives the same bytes every time.  No kernel waits on another
 * thread.  All arithmetic is fp64 (fp32 inputs widened first), every operation rounded separately (no FMA, no matrix instruction).
 *   mofa_shape_gram      P [R, N] (double, row-major), 1 <= R <= MOFA_SHAPE_MAX_ROWS;  weight [N / group] (double) or NULL;  group 1 or 3.
 *                        partial [ceil(N / MOFA_ICP_CHUNK), R (R + 1) / 2] (double): pair (a, b), a <= b, sits at a R - a (a - 1) / 2 + (b - a)
 *                        (the upper triangle row by row).  Column j of pair (a, b) has the term
 *                          term_j = weight[j / group] * (P[a][j] * P[b][j])        (weight NULL:  term_j = P[a][j] * P[b][j])
 *                        and a column whose weight is not `> 0` adds nothing, whatever P holds there (NaN, inf).  Chunk k holds the columns
 *                        [1024 k, min(1024 (k + 1), N)): thread t of its 256 starts at 0.0 and adds the terms of the chunk's columns t,
 *                        t + 256, t + 512, t + 768 (those below N) in that order; then `for w = 128, 64, .. 1: p[t] += p[t + w] for t < w`
 *                        over the 256 partial sums, and p[0] is the chunk's number: mofa_icp_reduce's sum of the [N, R (R + 1) / 2] matrix
 *                        of the terms, without that matrix.  The caller reduces the chunk rows with mofa_shape_reduce until one is left.
 *   mofa_shape_reduce    mofa_icp_reduce for rows of any width: out [ceil(M / MOFA_ICP_CHUNK), ncols] from in [M, ncols] (double),
 *                        1 <= ncols <= 32,896, the same additions in the same order.  in != out.
 *   mofa_shape_centre    meshes [M, n] (float), 1 <= M <= MOFA_SHAPE_MAX_ROWS:  s = 0.0;  s += (double)meshes[m][j]  (m ascending);
 *                        mean[j] = s / (double)M;   X[m][j] = (double)meshes[m][j] - mean[j].   mean [n], X [M, n] (double).
 *   mofa_shape_combine   out [B, n] (double) from coef [B, R] and rows [R, n] (double):  acc = 0.0;  acc += coef[b][r] * rows[r][j]
 *                        (r ascending);  out[b][j] = base[j] + acc  (base [n] double), or acc with base NULL.  1 <= B <= 65,535.
 *   mofa_shape_plane_rows   P [K + 1, V] (double) for the model's vertices i (moved [V,3], their closest points closest [V,3], both float,
 *                        face [V] int32 on the target mesh verts [TV,3] / faces [TF,3]):  n = the unit normal of faces[face[i]] exactly as
 *                        mofa_icp_terms takes it;  with transform = [s, R (row-major 3 x 3), t] (13 doubles, HOST; t unused)
 *                          q_c = s * ((R[0][c] * n_x + R[1][c] * n_y) + R[2][c] * n_z)     (s R^T n: the normal in the model's frame)
 *                          P[k][i] = (q_x * m_x + q_y * m_y) + q_z * m_z,   m = modes[k][i]   (modes [K, V, 3] double;  0 <= K < 256)
 *                          P[K][i] = (n_x * d_x + n_y * d_y) + n_z * d_z,   d = (double)moved[i] - (double)closest[i]
 *                        A face or vertex index outside the mesh writes NaN into column i of all K + 1 rows (the caller gives it weight 0).
 * A null pointer or a count out of range returns MOFA_EINVAL with a message. */
#define MOFA_SHAPE_MAX_ROWS 256
int mofa_shape_gram(const double* P, int32_t R, int64_t N, const double* weight, int32_t group, double* partial, void* stream);
int mofa_shape_reduce(const double* in, int64_t M, int64_t ncols, double* out, void* stream);
int mofa_shape_centre(const float* meshes, int32_t M, int64_t n, double* mean, double* X, void* stream);
int mofa_shape_combine(const double* base, const double* coef, const double* rows, int32_t B, int32_t R, int64_t n, double* out, void* stream);
int mofa_shape_plane_rows(const float* moved, const float* closest, const int32_t* face, const float* verts, int64_t TV, const int32_t* faces,
                          int64_t TF, const double transform[13], const double* modes, int32_t K, int64_t V, double* P, void* stream);

/* ---- occupancy-culled rendering: skip the network where an occupancy grid says the space is empty ---------------------------------
 * The grid lives on the lattice of mofa_grid_points (nx x ny x nz samples at lo + (i,j,k) step): (nx-1)(ny-1)(nz-1) cells, one byte
 * each (0 / 1), cell index (i (ny-1) + j) (nz-1) + k.  The lattice needs 2 <= n < 2^24 per axis and fewer than 2^31 cells.
 *   mofa_occ_cells   cells[c] = 1 iff one of the cell's 8 corner samples of grid [nx,ny,nz] is > threshold (NaN is not); merge != 0 ORs
 *                    into what cells already holds (the union over several networks).  The threshold must be finite.
 *   mofa_occ_dilate  out[c] = 1 iff a cell within Chebyshev distance `dilate` (0 .. 8, clipped at the borders) of c is set in cells:
 *                    a separable maximum, three passes through `scratch`; cells, scratch and out are three different buffers of one
 *                    byte per cell.
 * A pass of n_rays x S samples (fewer than 2^31), sample e = r S + s at p = o_r + d_r z_{r,s} with the multiply and the add rounded
 * separately (the point mofa_net_forward forms); z [n_rays,S] (z_row_stride = S) or one shared row (stride 0).  Per axis, in fp32:
 * t = (p - lo) / step (correctly rounded), inside = t >= 0 && t <= (float)(n - 1) (NaN: outside), c = min((int)t, n - 2).  A sample is
 * KEPT iff it is inside on all three axes and its cell is set.
 *   mofa_occ_classify  flags[e] = kept (one byte per sample); the 64-bit exclusive scan of the flags goes to `workspace`
 *                      (mofa_occ_workspace_bytes(n_rays S) bytes) and counts[0] = n_kept (int64, DEVICE).  lo / step: HOST arrays
 *                      (finite, step > 0).
 *   mofa_occ_gather    with the same pass, flags and workspace afterwards, n_kept = the host's copy of counts[0] (>= 1): the kept samples
 *                      in ascending e — pts [n_kept,3] (their points), dirs [n_kept,3] (their rays' view directions), index [n_kept]
 *                      (int32: e).  What mofa_net_forward takes as explicit points with S = 1.
 *   mofa_occ_scatter   raw [n_samples,4] = raw_kept [n_kept,4] row scan[e] for a kept sample, (0,0,0,0) for a skipped one: every
 *                      element is written by this one kernel.  raw_kept may be NULL when n_kept = 0.  Both 16-byte aligned.
 * No atomics: the same input gives the same bytes.  A slot at or beyond n_kept (a count that does not belong to the flags) is never
 * written by gather and gives NaN in scatter. */
size_t mofa_occ_workspace_bytes(int64_t n_samples);   /* 0 for n_samples < 1 or >= 2^31 */
int mofa_occ_cells(const float* grid, int64_t nx, int64_t ny, int64_t nz, float threshold, int32_t merge, uint8_t* cells, void* stream);
int mofa_occ_dilate(const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, int32_t dilate, uint8_t* scratch, uint8_t* out, void* stream);
int mofa_occ_classify(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S,
                      const uint8_t* cells, int64_t nx, int64_t ny, int64_t nz, const float lo[3], const float step[3], uint8_t* flags,
                      void* workspace, int64_t* counts, void* stream);
int mofa_occ_gather(const float* rays_o, const float* rays_d, const float* viewdirs, const float* z, int64_t z_row_stride, int64_t n_rays,
                    int32_t S, const uint8_t* flags, const void* workspace, int64_t n_kept, float* pts, float* dirs, int32_t* index,
                    void* stream);
int mofa_occ_scatter(const float* raw_kept, const uint8_t* flags, const void* workspace, int64_t n_samples, int64_t n_kept, float* raw,
                     void* stream);

/* The one-float twin of mofa_occ_scatter (the geometry-only render): sigma [n_samples] = sigma_kept [n_kept] entry scan[e] for a kept
 * sample, 0 for a skipped one; every element is written by this one kernel, a slot at or beyond n_kept gives NaN.  sigma_kept may be NULL
 * when n_kept = 0. */
int mofa_occ_scatter_sigma(const float* sigma_kept, const uint8_t* flags, const void* workspace, int64_t n_samples, int64_t n_kept,
                           float* sigma, void* stream);

/* ---- backward (run_fit.py:305-313 photometric fitting, run_train.py:333-357 training) -----------------------
 * Backward of mofa_net_forward given d_raw [n_rays,S,4] and the tape (fp32, or mask-only when d_weights == NULL) of that forward:
 *   d_folded  [mofa_net_folded_floats]: gradient w.r.t. every folded bias (sum over points of the ReLU-masked
 *             pre-activation gradient) — host autograd carries it on to the codes / raw biases / constant columns;
 *   d_view_bias_rows [n_rays, roundup(W/2,64)]: gradient w.r.t. the per-ray view bias rows;
 *   d_rays_o, d_rays_d [n_rays,3]: through the positional encoding and pts = o + d*z (z carries no gradient: the
 *             coarse z is constant and the fine z is detached, render_class.py:326);
 *   or, when the forward ran on explicit points (`pts` != NULL — run_network(inputs, viewdirs, fn) under autograd,
 *             render_class.py:69-94): d_pts [n_rays*S,3]; rays_o / rays_d / z / d_rays_o / d_rays_d are then unused (NULL).
 * packed_t: transposed weight panels from mofa_net_pack_t; workspace: mofa_net_backward_workspace_floats(). */
size_t mofa_net_packed_t_floats(MofaNetShape s);
size_t mofa_net_tape_floats(MofaNetShape s, int64_t n_points);
size_t mofa_net_mask_tape_words(MofaNetShape s, int64_t n_points);   /* uint64 words = tape floats / 64 */
size_t mofa_net_backward_workspace_floats(MofaNetShape s, int64_t n_points, int32_t with_weight_grads);   /* d_weights != NULL (training) or not (fitting): the two forms keep different buffers */
int mofa_net_pack_t(MofaNetShape s, const float* const* weights, float* packed_t, void* stream);
int mofa_net_backward(MofaNetShape s, const float* packed, const float* packed_t, const float* tape, const uint64_t* mask_tape,
                      const float* d_raw, const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride,
                      const float* pts, int64_t n_rays, int32_t S, float* workspace, float* d_folded,
                      float* d_view_bias_rows, float* d_rays_o, float* d_rays_d, float* d_pts, float* const* d_weights, uint32_t* verdict,
                      void* stream);
/* d_weights: NULL (fitting: only codes/pose are optimised), or 2D+7 pointers to [out,in] gradient tensors in state-dict
 * order: the per-point column blocks are OVERWRITTEN with dW = G^T X (fp32 MFMA, contraction over the points, split over
 * M with a deterministic second-stage sum); the per-call-constant columns are left untouched (host autograd owns them). */
size_t mofa_weight_grad_workspace_floats(int64_t n_points, int32_t n_padded, int32_t k_padded);
int mofa_weight_grad(const float* g, int32_t n_padded, const float* x, int32_t k_padded, int64_t m_padded,
                     int64_t n_points, int32_t n_out, int32_t ncols, float* dst, int32_t ld, int32_t col0,
                     float* bias_out /* NULL or [n_padded] = sum_m G[m][:] from the same pass */, float* workspace,
                     void* stream);
int mofa_head_weight_grad(const float* d_raw, int32_t raw_off, int32_t n_out, const float* x, int32_t k_padded,
                          int64_t m_padded, int64_t n_points, int32_t ncols, float* dst, int32_t ld, void* stream);
/* positional-encoding features of every point (o + d z, or explicit `pts`) as panels [mofa_pe_k_padded(n_freqs)/16][m_padded][16] */
int mofa_pe_panels(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, const float* pts, int64_t n_points,
                   int32_t S, int32_t n_freqs, int64_t m_padded, float* out, void* stream);
/* pieces of mofa_net_backward (unit-testable) */
int mofa_pack_panels_t(const float* w, int32_t n_out, int32_t ld, int32_t col0, int32_t ncols, float* dst,
                       int32_t rows_padded, int32_t k_padded, void* stream);
/* mask: the saved fp32 activation (dx *= mask > 0).  _bits: the same mask as ONE BIT per activation — the mask-only tape's layout:
 * float offset o of the dx-shaped panel buffer <-> bit ((o & 255) >> 2) of 64-bit word (o >> 8) * 4 + (o & 3). */
int mofa_layer_backward_data(const float* g, int32_t g_k, const float* wt_packed, const float* mask, int32_t accumulate,
                             float* dx, int64_t m_padded, int32_t k_out_padded, void* stream);
int mofa_layer_backward_data_bits(const float* g, int32_t g_k, const float* wt_packed, const uint64_t* mask_bits, int32_t accumulate,
                                  float* dx, int64_t m_padded, int32_t k_out_padded, void* stream);
int mofa_head_backward(const float* d_raw, int32_t raw_off, int32_t n_out, const float* w_dense, int32_t k_padded,
                       const float* mask, int32_t accumulate, float* dx, int64_t m_padded, int64_t n_points, void* stream);
int mofa_head_backward_bits(const float* d_raw, int32_t raw_off, int32_t n_out, const float* w_dense, int32_t k_padded,
                            const uint64_t* mask_bits, int32_t accumulate, float* dx, int64_t m_padded, int64_t n_points, void* stream);
int mofa_bias_grad(const float* g, int64_t m_padded, int64_t n_points, int32_t n_padded, float* out, void* stream);
int mofa_bias_grad_rays(const float* g, int64_t m_padded, int64_t n_rays, int32_t S, int32_t n_padded, float* out,
                        void* stream);
int mofa_pe_backward(const float* dpe, int64_t m_padded, const float* rays_o, const float* rays_d, const float* z,
                     int64_t z_row_stride, int64_t n_rays, int32_t S, int32_t n_freqs, float* d_rays_o, float* d_rays_d, void* stream);
int mofa_pe_backward_points(const float* dpe, int64_t m_padded, const float* pts, int64_t n_points, int32_t n_freqs, float* d_pts,
                            void* stream);
/* raw2outputs backward: upstream gradients g_* (g_disp/g_acc/g_depth/g_weights may be NULL = zero) ->
 * d_raw [n_rays,S,4] and the |rays_d| contribution d_rays_d [n_rays,3] (may be NULL). */
int mofa_composite_backward(const float* raw, const float* z, int64_t z_row_stride, const float* rays_d,
                            const float* noise, int64_t n_rays, int32_t S, int32_t white_bkgd, const float* g_rgb,
                            const float* g_disp, const float* g_acc, const float* g_depth, const float* g_weights,
                            float* d_raw, float* d_rays_d, void* stream);

/* ---- single-layer entry points (unit-testable pieces of mofa_net_forward) -------------------- */
size_t mofa_panel_floats(int64_t rows, int32_t k); /* rows * roundup(k,16) */
int mofa_pack_panels(const float* w, int32_t n_out, int32_t ld, int32_t col0, int32_t ncols, float* dst,
                     int32_t rows_padded, int32_t panel0, int32_t k_padded, void* stream);
int mofa_to_panels(const float* x, int64_t rows, int32_t k, float* dst, int64_t rows_padded, void* stream);
int mofa_from_panels(const float* src, int64_t rows_padded, int64_t rows, int32_t k, float* x, void* stream);
/* y = act(x1|x2 @ Wpacked^T + bias); bias_row_div = 0: bias[Np]; else bias[(m / div), Np] (per ray).
 * _masked: mask_bits_out = NULL, or m_padded * n_padded / 64 words receiving (y > 0) as bits (mask-only tape; requires relu). */
int mofa_layer_forward(const float* x1, int32_t k1, const float* x2, int32_t k2, const float* w_packed,
                       const float* bias, int32_t bias_row_div, int64_t bias_rows, float* y, int64_t m_padded,
                       int32_t n_padded, int32_t relu, void* stream);
int mofa_layer_forward_masked(const float* x1, int32_t k1, const float* x2, int32_t k2, const float* w_packed,
                              const float* bias, int32_t bias_row_div, int64_t bias_rows, float* y, int64_t m_padded,
                              int32_t n_padded, int32_t relu, uint64_t* mask_bits_out, void* stream);
/* first layer with the positional encoding (n_freqs = multires) generated in the prologue (model.py:44-45 + Linear0);
 * w_packed: mofa_pe_k_padded(n_freqs) / 16 panels. */
int mofa_layer0_forward(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride,
                        const float* pts, int64_t n_points, int32_t S, int32_t n_freqs, const float* w_packed, const float* bias,
                        float* y, int64_t m_padded, int32_t n_padded, uint64_t* mask_bits_out, void* stream);
/* Layer 0 with ray generation FOLDED INTO THE PROLOGUE: the ray of point m is built from
 * (intrinsics, c2w[3,4], pixel) by the arithmetic of mofa_get_rays — pixel = pixels[m / S] (flat row * img_w + col) or
 * pix0 + m / S when pixels == NULL — then pts = o + d * z as in mofa_layer0_forward.  Bit-identical to
 * mofa_get_rays(_at) followed by mofa_layer0_forward.  (The shipped renderer keeps the 24 B / ray arrays because compositing and
 * the positional-encoding backward read them as well; this entry is the kernel-level form.) */
int mofa_layer0_forward_cam(int32_t img_w, float fx, float fy, float cx, float cy, const float* c2w, const int32_t* pixels,
                            int64_t pix0, const float* z, int64_t z_row_stride, int64_t n_points, int32_t S, int32_t n_freqs,
                            const float* w_packed, const float* bias, float* y, int64_t m_padded, int32_t n_padded, void* stream);
int mofa_head_forward(const float* x, int32_t k_padded, int64_t m_padded, const float* w_dense, const float* b,
                      int32_t n_out, float* raw, int32_t raw_off, int64_t n_points, void* stream);
/* out[r][n] = bias[n] + sum_k w[n][k] * PE(viewdirs[r])[k], k < 3 + 6 * n_freqs (n_freqs = multires_views) */
int mofa_view_bias(const float* viewdirs, int64_t n_rays, int32_t n_freqs, const float* w, int32_t n_out, int32_t ld,
                   const float* bias, float* out, int32_t n_padded, void* stream);
int mofa_positional_encode(const float* x, int64_t n, int32_t n_freqs, float* out, void* stream);

/* ---- measurement hook ------------------------------------------------------------------------
 * A measurement session of the CALLING THREAD'S CURRENT DEVICE (state is per device, mutex-guarded; with no session
 * open the launch paths read one atomic flag).  Between mofa_prof_begin() and mofa_prof_end() every launch of the kernels below is
 * bracketed by hipEventRecord on its own stream.  mofa_prof_end() synchronises those events (host blocks) and fills three arrays of
 * length MOFA_PROF_KINDS: summed kernel time, launch count, WORK executed.
 *   MFMA kernels (work = FLOPs, 2*M*K*N of the padded shapes):
 *     [0] the per-layer forward kernel k_layer<128,..,PIPE> (128-feature tile, pipelined K loop)   [1] the persistent whole-network
 *     kernel k_mlp_fused (widths <= 256)   [2] the backward-data kernel k_layer<128,..,BWD>   [3] the weight-gradient kernel k_wgrad
 *     [4] the view layer's per-ray-bias instantiation of the forward kernel   [5] the chained wide-network kernel k_net_chain<0>
 *     (forward: inference or keeping the fp32 tape)   [6] k_net_chain<2> (the fitting backward's backward-data products)
 *     [7] k_net_chain<1> (forward, also writing the mask tape)   [11] k_net_chain_train (the training backward of a wide network as
     chained launches: backward-data products and weight gradients)
 *   HBM-bound ray kernels (work = RAYS; bench.py multiplies by SURVEY section 8d's algorithmic bytes per ray):
 *     [8] k_composite<1> (S <= 64: the coarse pass)   [9] k_composite<2> (S <= 128: the fine pass)   [10] k_sample_pdf_merge
 * Used by bench.py only. */
#define MOFA_PROF_KINDS 12
int mofa_prof_begin(void);
int mofa_prof_end(double* total_ms, int64_t* launches, double* padded_flops);

/* ---- ray-side kernels ------------------------------------------------------------------------ */
/* get_rays (tools/run_nerf_helpers.py:153-168) + viewdir normalisation (render_class.py:399-401) for
 * pixels [pix0, pix0+n) of an H x W image in row-major order.  c2w: 12 floats [3,4] (device). */
int mofa_get_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w, int64_t pix0,
                  int64_t n, float* rays_o, float* rays_d, float* viewdirs, void* stream);

/* The same for a LIST of pixels (flat indices row * W + col, int32, device): the rays of a fitting / training batch without
 * building the H x W grid first (run_fit.py:281-293 builds get_rays_withGrad's full grid and gathers N_rand of it;
 * run_train.py:306-330).  Bit-identical to mofa_get_rays at those pixels. */
int mofa_get_rays_at(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w, const int32_t* pixels,
                     int64_t n, float* rays_o, float* rays_d, float* viewdirs, void* stream);

/* Reverse of ray generation — the camera-pose gradient run_fit.py optimises (get_rays_withGrad, run_fit.py:116-127):
 *   d_c2w[a][b] = sum_rays d_rays_d[ray][a] * dirs[ray][b] (b < 3),  d_c2w[a][3] = sum_rays d_rays_o[ray][a];  d_c2w: 12 floats.
 * pixels == NULL: the contiguous pixel range [pix0, pix0 + n).  Deterministic (fixed-order double sums, no atomics). */
int mofa_rays_pose_backward(int32_t W, float fx, float fy, float cx, float cy, const int32_t* pixels, int64_t pix0, int64_t n,
                            const float* d_rays_o, const float* d_rays_d, float* d_c2w, void* stream);

/* raw2outputs (render_class.py:440-482): one wavefront per ray, exclusive prefix product over the
 * samples.  noise may be NULL; disp is NaN where acc == 0 exactly like the reference. */
int mofa_composite_forward(const float* raw, const float* z, int64_t z_row_stride, const float* rays_d,
                           const float* noise, int64_t n_rays, int32_t S, int32_t white_bkgd, float* rgb,
                           float* disp, float* acc, float* depth, float* weights, void* stream);

/* ---- geometry-only render: depth, silhouette and disparity from the density alone ---------------------------
 * pts [n_rays*S,3]: pts[r S + s] = o_r + d_r * z_{r,s}, the multiply and the add rounded separately — the point mofa_net_forward forms
 * in its layer-0 prologue and mofa_occ_gather forms for a kept sample; what mofa_net_density takes.  z [n_rays,S] (z_row_stride = S) or
 * one shared row (stride 0); at least one and fewer than 2^31 samples. */
int mofa_ray_points(const float* rays_o, const float* rays_d, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S,
                    float* pts, void* stream);

/* raw2outputs without colour: sigma [n_rays,S] is the pre-ReLU density (raw[..., 3]) on its own; noise may be NULL.  Writes disp, acc,
 * depth [n_rays] and weights [n_rays,S] (required: the resampler's input) — each the same bits mofa_composite_forward gives for a raw
 * whose channel 3 is sigma (same lane-to-sample assignment, same operations in the same order).  S >= 2, z_row_stride 0 or S, fewer
 * than 2^31 samples. */
int mofa_composite_sigma(const float* sigma, const float* z, int64_t z_row_stride, const float* rays_d, const float* noise,
                         int64_t n_rays, int32_t S, float* disp, float* acc, float* depth, float* weights, void* stream);

/* Median termination depth of a ray from its compositing weights [n_rays,S]: index[r] (int32) = the least i whose inclusive prefix sum
 * C_i = w_0 + ... + w_i reaches `threshold` (C_i >= threshold), depth_med[r] = z[r][index[r]]; when no C_i reaches it (a ray through
 * empty space; a NaN weight in front of the crossing) index = -1 and depth_med = z[r][S-1].  Every C_i is an fp32 sum of exactly
 * w_0..w_i (one wavefront per ray: in-lane running sums under a wavefront scan), so it lies within (S-1) 2^-24 sum|w| of the exact sum.
 * z as above (stride S or 0); S >= 1, fewer than 2^31 samples; threshold finite and > 0. */
int mofa_depth_median(const float* weights, const float* z, int64_t z_row_stride, int64_t n_rays, int32_t S, float threshold,
                      float* depth_med, int32_t* index, void* stream);

/* Screen-space normals of a point map: points [H,W,3], acc [H,W], rays_d [H,W,3] -> normals [H,W,3], valid [H,W] (uint8).  A pixel is
 * usable iff acc >= acc_min (NaN is not).  Along each image axis the difference is central (P[+1] - P[-1]) when both neighbours exist and
 * are usable, else forward (P[+1] - P), else backward (P - P[-1]), else the pixel is invalid.  n = du x dv (du along columns, dv along
 * rows; products and subtraction rounded separately), len = sqrt((nx nx + ny ny) + nz nz) correctly rounded, invalid unless len > 0, n / len, negated
 * where (nx dx + ny dy) + nz dz > 0 so that normals face the camera.  Every element is written: unusable or invalid pixels get (0,0,0)
 * and valid = 0 (a 1 x W or H x 1 map comes out all invalid).  Fewer than 2^31 pixels; acc_min finite. */
int mofa_point_normals(const float* points, const float* acc, const float* rays_d, int32_t H, int32_t W, float acc_min, float* normals,
                       uint8_t* valid, void* stream);

/* sample_pdf on (z_mid, weights[1:-1]) + sort(cat(z, z_samples)) + std(z_samples)
 * (render_class.py:324-328,345; tools/run_nerf_helpers.py:203-247).  u: [n_rays,Ni] (stride Ni) or a
 * shared row (stride 0) — linspace(0,1,Ni) for det.
 * The arithmetic, one fp32 rounding per operation (no fused multiply-add, correctly rounded division): bins_i = 0.5f * (z[i+1] + z[i]);
 * wp = w + 1e-5f over the interior weights w[1 .. S-2] (w[0] and w[S-1] are not read); wsum = (float)(fp64 sum of wp); pdf = wp / wsum;
 * cdf_0 = 0, cdf_k = (float)(fp64 sum of pdf_0 .. pdf_{k-1}); lo = the first index with cdf > u, below = max(lo - 1, 0),
 * above = min(lo, B - 1); den = cdf[above] - cdf[below], replaced by 1 when < 1e-5f; t = (u - cdf[below]) / den;
 * z_samples = bins[below] + t * (bins[above] - bins[below]).  z_std = (float)sqrt of the fp64 population variance of the row's samples
 * (0 for Ni = 1).  A NaN interior weight makes every sample of its ray, and z_std, NaN.
 * z_fine is the STABLE sort of cat(z, z_samples) along the ray: equal values keep their order in the concatenation, every NaN comes
 * after every number, NaNs in their order in the concatenation (torch.sort's order).  Every slot of z_fine is written for any input. */
int mofa_sample_pdf_merge(const float* z, int64_t z_row_stride, const float* weights, const float* u,
                          int64_t u_row_stride, int64_t n_rays, int32_t S, int32_t Ni, float* z_samples,
                          float* z_fine, float* z_std, void* stream);

/* sample_pdf(bins, weights, N_samples, det / u) exactly as tools/run_nerf_helpers.py:203-247 takes it: bins [n_rays, n_bins]
 * (row stride given; 0 = one shared row), weights [n_rays, n_bins-1], u as above -> samples [n_rays, Ni].  Same kernel as
 * mofa_sample_pdf_merge without the mid-point / merge stages; this is the form the reference's own KATs are stated in. */
int mofa_sample_pdf(const float* bins, int64_t bins_row_stride, const float* weights, const float* u, int64_t u_row_stride,
                    int64_t n_rays, int32_t n_bins, int32_t Ni, float* samples, void* stream);

/* ---- mesh rasteriser: depth, face index, barycentrics, attributes and flat normals of a triangle mesh ------------------------
 * verts [n_verts,3] fp32 (world), faces [n_faces,3] int32, c2w [3,4] row-major (DEVICE, as mofa_get_rays takes it), pinhole fx, fy, cx, cy.
 * The camera is the one of mofa_get_rays: pixel (i, j) (column, row) is sampled at the integer point (i, j), the camera looks along -z,
 * and `depth` is the ray parameter of that pixel's ray — the quantity mofa_composite_sigma / mofa_depth_median give without NDC.
 *   vertex    d = v - t, p_a = (d0 c[0][a] + d1 c[1][a]) + d2 c[2][a], zc = -p_2, u = cx + fx (p_0 / zc), v = cy - fy (p_1 / zc), every
 *             operation rounded separately; valid iff zc >= znear, |u| <= 2^20 and |v| <= 2^20 (false for NaN); X = rint(256 u), Y = rint(256 v)
 *   face      culled whole when a corner is invalid or an index lies outside [0, n_verts) (no near-plane clipping); degenerate when
 *             A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) is 0; otherwise drawn, either winding
 *   coverage  int64 edge functions at (256 i, 256 j): w0 = s E(1,2), w1 = s E(2,0), w2 = s E(0,1), s = sign(A),
 *             E(p,q) = (Xq-Xp)(Py-Yp) - (Yq-Yp)(Px-Xp); covered iff all three >= 0 (a sample on a shared edge belongs to both faces)
 *   depth     fp64, rounded once: l_k = w_k / |A|, q = (l0/z0 + l1/z1) + l2/z2, depth = (float)(1/q), b_k = (l_k/z_k)/q,
 *             attr_c = (float)((b0 a0c + b1 a1c) + b2 a2c)
 *   pixel     the least (depth bits << 32 | face) over the faces that cover it (64-bit atomicMin on a z-buffer in the workspace): the
 *             nearest face, the lower index at equal depth bits — whatever the order of the atomics
 *   normal    n = (v1-v0) x (v2-v0) in the operation order of mofa_point_normals, (0,0,0) unless its length is > 0, n / len, negated
 *             where n . d > 0 for the pixel's ray direction d
 * Call order per frame, on one stream: project, faces, resolve (any number of resolves).  No call synchronises the host. */
size_t mofa_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int32_t H, int32_t W);   /* 0 when refused: H or W < 1, H W >= 2^31,
                                                                                                 a negative count, n_verts or n_faces >= 2^31 */
/* one lane per vertex: snapped screen position, camera depth and validity into the workspace.  znear finite and > 0. */
int mofa_raster_project(const float* verts, int64_t n_verts, int64_t n_faces, int32_t H, int32_t W, float fx, float fy, float cx, float cy,
                        const float* c2w, float znear, void* workspace, void* stream);
/* clears the z-buffer and rasterises.  A face whose clipped box of samples holds fewer than wave_min_pixels (>= 0) pixels is walked by
 * one lane, the others one wavefront per face (0: every face by a wavefront; INT32_MAX: every face by a lane) — the same bits either way.
 * counts [4] int64 (DEVICE): faces drawn, culled, degenerate, and drawn faces that took the wavefront path.  n_faces or n_verts = 0 is
 * valid: an empty frame. */
int mofa_raster_faces(const int32_t* faces, int64_t n_faces, int64_t n_verts, int32_t H, int32_t W, int32_t wave_min_pixels, void* workspace,
                      int64_t* counts, void* stream);
/* one lane per pixel: depth [H,W], face [H,W] (int32) and, where not NULL, bary [H,W,3], attr_out [H,W,C] (attrs [n_verts,C], C in 1 .. 16)
 * and normal [H,W,3].  Every element is written; an uncovered pixel gets depth 0, face -1 and zeros. */
int mofa_raster_resolve(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* attrs, int32_t C, int32_t H,
                        int32_t W, float fx, float fy, float cx, float cy, const float* c2w, const void* workspace, float* depth, int32_t* face,
                        float* bary, float* attr_out, float* normal, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MOFANERF_HIP_H */
