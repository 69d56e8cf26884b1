// The host side of a pass: what one calc_H_g_e2 / one align / one batch puts on the stream and how it waits for the result
// (Pass, pass_setup, pass_enqueue = enqueue_fused | enqueue_search + enqueue_reduce, pcr_run_linearize / _align / _batch / _rows / _nn).  No kernel lives here and no kernel template is
// named: every launch goes through the launch_* functions of kernels.hip (pass_device.h), so an edit of this file compiles in
// seconds.
#include <stdlib.h>

#include "pass_device.h"

// blocks of a pass kernel: `want` rounded up to a multiple of 8 (one contiguous span of the scan per XCD; TileIter and the
// ticket counts of the folds need it), at most `cap` rounded down to one, at least 8
static int grid8(int64_t want, int64_t cap = INT64_MAX) {
    int64_t nb = (want + 7) & ~(int64_t)7;
    if (nb > (cap & ~(int64_t)7)) nb = cap & ~(int64_t)7;
    return nb < 8 ? 8 : (int)nb;
}

#define PCR_HOST_ROWS_BYTES (sizeof(double) * 8 * 32 + sizeof(uint32_t) * 8 * PCR_GFLAG_STRIDE)

static double cell_edge(const pcr_target *t) { return t->is_voxel ? t->gd.h : (double)t->gf.h; }

pcr_status pcr_ensure_scratch(pcr_context *ctx, int64_t n_points) {
    (void)n_points;
    if (!ctx->d_partials) {
        ctx->max_blocks = (ctx->num_cu * 16 + 7) & ~7;
        // + 8 rows: the group sums of k_reduce_finalize live behind the per-block rows
        HIP_TRY(pcr_malloc_retry((void **)&ctx->d_partials, sizeof(double) * 32 * (size_t)(ctx->max_blocks + 8)));
        HIP_TRY(pcr_malloc_retry((void **)&ctx->d_out, sizeof(double) * 32));
        HIP_TRY(pcr_malloc_retry((void **)&ctx->d_pose, sizeof(PoseDev)));
        // pinned + mapped: [0..28] sums, [32] sequence number (pcr_linearize); [40..55] pose, [56] loop state (pcr_align)
        HIP_TRY(hipHostMalloc(&ctx->h_out, sizeof(double) * 64, hipHostMallocMapped | hipHostMallocCoherent));
        memset(ctx->h_out, 0, sizeof(double) * 64);
        HIP_TRY(hipHostGetDevicePointer((void **)&ctx->h_out_dev, ctx->h_out, 0));
        // host fold: 8 group rows of 32 doubles, then the 8 group sequence words (PCR_GFLAG_STRIDE words apart)
        HIP_TRY(hipHostMalloc((void **)&ctx->h_rows, PCR_HOST_ROWS_BYTES, hipHostMallocMapped | hipHostMallocCoherent));
        memset(ctx->h_rows, 0, PCR_HOST_ROWS_BYTES);
        HIP_TRY(hipHostGetDevicePointer((void **)&ctx->h_rows_dev, ctx->h_rows, 0));
        // 8 + 1 tickets (a 128-byte line each), then the tile counters
        // ... then the word of k_nn_fix (the stamp of the last filter pass that left work for it)
        const size_t ctr_words = 9 * PCR_TICKET_STRIDE + (size_t)PCR_TILE_CTRS * PCR_TILE_STRIDE + 16;
        HIP_TRY(pcr_malloc_retry((void **)&ctx->d_tile_ctr, sizeof(uint32_t) * ctr_words));
        HIP_TRY(hipMemsetAsync(ctx->d_tile_ctr, 0, sizeof(uint32_t) * ctr_words, ctx->stream));
        auto blocks_per_cu = [](int which, int fallback) { const int nb = nn_blocks_per_cu(which); return nb > 0 ? nb : fallback; };
#ifdef PCR_DEV
        ctx->nn_blocks_per_cu[4] = blocks_per_cu(PCR_OCC_MFMA, 2);
        ctx->nn_blocks_per_cu[2] = pcr_dev_coop_blocks_per_cu();
#endif
        ctx->nn_blocks_lb = blocks_per_cu(PCR_OCC_POINT_LB, 4);
        ctx->nn_blocks_per_cu[0] = blocks_per_cu(PCR_OCC_POINT, 4);
        ctx->nn_blocks_per_cu[1] = blocks_per_cu(PCR_OCC_VOXEL, 4);
        ctx->nn_blocks_per_cu[3] = blocks_per_cu(PCR_OCC_FILTER, 4);
    }
    return PCR_OK;
}

// enough 256-thread blocks to fill every CU several times over, never more than the work
static int64_t blocks_wanted(const pcr_context *ctx, int64_t n) {
    const int64_t want = (n + 255) / 256, cap = (int64_t)ctx->num_cu * 8;
    return want < cap ? want : cap;
}
int choose_blocks(const pcr_context *ctx, int64_t n) { return grid8(blocks_wanted(ctx, n), ctx->max_blocks); }   // (odd CU counts round down)

// ---- one pass = NN kernel + reduce kernel (variant 1) or the fused kernel (variant 0) ------------
struct Pass {
    pcr_context *ctx;
    pcr_target *t;
    pcr_scan *s;
    int kind;
    LinArgs a;
    FinArgs f;
    bool one_kernel;     // fused search + reduce kernel (variant 0, or variant 2 on a small scan)
    bool fused_fin;      // the fold of the block partials inside the producing kernel instead of k_finalize
    bool gn_inline;      // device-resident loop, fused kernel, one GPU: the Gauss-Newton step runs inside the fused kernel
    double motion;       // typical displacement of the scan since the previous pass over it (host-driven passes; -1 unknown)
    bool list_force;     // PCR_LIST_SET put one deeper list set in place of both (pass_fill_lin)
    int nn_mode;         // PCR_NN_FULL / TRACK / LIST
    bool reuse_ready;    // the scan has the buffers of the certified-reuse path
    bool q6;             // PlaneICP pass over a float64 point target: float64 search (quirk Q6, pcr_target::pts64)
};

bool pcr_pass_is_fused(const pcr_context *ctx, const pcr_scan *s) {
    if (ctx->variant == 2) return s->n <= (int64_t)ctx->num_cu * 1024;   // measured crossover: 262 k - 350 k points on 256 CUs
    return ctx->variant == 0;
}

static void set_filter_bound(LinArgs &a, double bound);
// (bits 27-29 of LinArgs::flags are internal -- the gate switch of quirk Q6, two developer timing switches; a
// caller-supplied word must not reach them)
#define PCR_PUBLIC_FLAGS (PCR_FLAG_ICP_RR_QUIRK | PCR_FLAG_NO_SCAN_SORT | PCR_FLAG_LOCAL_ONLY | PCR_FLAG_HOST_LOOP | PCR_FLAG_DEVICE_LOOP | PCR_FLAG_KEEP_ORDER)

// quirk Q6: a PlaneICP pass over a float64 point target searches in float64 (pcr_target::pts64)
static bool pass_is_q6(const pcr_target *t, int kind) { return kind == PCR_PLANE && !t->is_voxel && t->pts64 != nullptr; }

// what the batched and the rows passes refuse: a communicator, and Q6 (the nouns and the note are the caller's, for the message)
static pcr_status refuse_comm_and_q6(const pcr_target *t, int kind, const char *passes, const char *plane_passes, const char *q6_note) {
    if (t->ctx->comm != nullptr) pcr_set_error("%s are not available on a context with a communicator attached (pcr_comm_*, pcr_group)", passes);
    else if (pass_is_q6(t, kind)) pcr_set_error("%s are not available over a float64 point target (%s)", plane_passes, q6_note);
    else return PCR_OK;
    return PCR_ERR_UNSUPPORTED;
}

// ---- pass_setup, step by step (in the order they run) ----
// what every Pass starts from (pass_setup, rows_search); reads the context only, touches neither the scan nor the target
static void pass_init(Pass *ps, pcr_target *t, pcr_scan *s, int kind, bool one_kernel, bool q6) {
    memset(ps, 0, sizeof *ps);
    ps->ctx = t->ctx; ps->t = t; ps->s = s; ps->kind = kind; ps->one_kernel = one_kernel; ps->q6 = q6;
#ifdef PCR_DEV
    ps->fused_fin = t->ctx->fuse_finalize;
#else
    ps->fused_fin = true;                       // (the unfused folds live in kernels_dev.hip: developer build only)
#endif
    ps->nn_mode = PCR_NN_FULL;
    ps->motion = -1.0;
}

static pcr_status pass_validate(const pcr_target *t, const pcr_scan *s, int kind, double max_dist) {
    PCR_REQUIRE(s->ctx == t->ctx, "scan and target belong to different contexts");
    PCR_REQUIRE(kind >= PCR_ICP && kind <= PCR_NDT, "unknown kind");
    PCR_REQUIRE(max_dist > 0, "max_dist must be positive");
    if ((kind == PCR_ICP || kind == PCR_PLANE) && t->is_voxel) {
        pcr_set_error("kind %d needs a point target", kind);
        return PCR_ERR_NO_TARGET;
    }
    if ((kind == PCR_VPLANE || kind == PCR_NDT) && !t->is_voxel) {
        pcr_set_error("kind %d needs a voxel target", kind);
        return PCR_ERR_NO_TARGET;
    }
    if (kind == PCR_PLANE && !t->pn) { pcr_set_error("PlaneICP target has no normals"); return PCR_ERR_NO_TARGET; }
    if (kind == PCR_VPLANE && !t->vnorm) { pcr_set_error("VPlaneICP target has no voxel normals"); return PCR_ERR_NO_TARGET; }
    if (kind == PCR_NDT && !t->vicov) { pcr_set_error("NDT target has no inverse covariances"); return PCR_ERR_NO_TARGET; }
    return PCR_OK;
}

// (nn_mode 4, developer build: plain searches run the MFMA-filtered kernel)
static bool nn_plain(const pcr_context *ctx) { return ctx->nn_mode == 0 || ctx->nn_mode == 4; }

// what a search + reduce pass keeps per scan point: the matches, and the buffers of certified reuse / the MFMA-filtered search
static pcr_status pass_scan_buffers(Pass *ps, int nblocks_split) {
    pcr_context *ctx = ps->ctx;
    pcr_scan *s = ps->s;
    ps->reuse_ready = false;
    if (ps->one_kernel) return PCR_OK;
    if (!s->nn_j) {
        HIP_TRY(pcr_scan_alloc(s, (void **)&s->nn_j, sizeof(uint32_t) * (size_t)(s->n > 0 ? s->n : 1)));
        s->nn_serial = 0;
    }
    if (!ps->q6 && ctx->reuse != 0 && (nn_plain(ctx) || ctx->nn_mode == 3) && s->n > 0) {
        if (!s->lb2 || !s->umask) {
            const size_t words = (((size_t)s->n + 63) / 64 + 31) & ~(size_t)15;     // whole 16-word chunks + slack
            if (!s->lb2) HIP_TRY(pcr_scan_alloc(s, (void **)&s->lb2, sizeof(float) * (size_t)s->n));
            HIP_TRY(pcr_scan_alloc(s, (void **)&s->umask, sizeof(unsigned long long) * words));
            HIP_TRY(hipMemsetAsync(s->umask, 0, sizeof(unsigned long long) * words, ctx->stream));
            s->track_valid = false;
        }
        if (s->ucnt_cap < nblocks_split) {
            pcr_scan_free(s, s->ucnt);
            s->ucnt = nullptr; s->ucnt_cap = 0;
            HIP_TRY(pcr_scan_alloc(s, (void **)&s->ucnt, sizeof(uint32_t) * (size_t)nblocks_split));
            s->ucnt_cap = nblocks_split;
        }
        ps->reuse_ready = true;
    }
    // the MFMA-filtered search (developer build) keeps its per-point bounds in lb2 (dead between passes unless the previous one
    // was a tracking pass, and a full search invalidates those anyway)
    if (!ps->q6 && !ps->t->is_voxel && ctx->nn_mode == 4 && !s->lb2 && s->n > 0) {
        HIP_TRY(pcr_scan_alloc(s, (void **)&s->lb2, sizeof(float) * (size_t)s->n));
        s->track_valid = false;
    }
    return PCR_OK;
}

// The filter index is built by the first pass that gets its cost back: a search + reduce pass at once; the fused
// small-scan kernel (which gains ~10 us per pass from it against ~0.3 ms of build) once the target has served
// PCR_FILTER_AFTER fused passes -- i.e. not during the one align() of the reference's benchmark protocol
// (set_target + align, benchmark/speed_test_comparison.py:36-55), but from the second align on for a map that stays
static void pass_lazy_filter(pcr_context *ctx, pcr_target *t, bool one_kernel) {
    if (t->filter_tried) return;
    if (one_kernel && ++t->fused_passes <= ctx->filter_after) return;
    t->filter_tried = true;
    // a failed build (out of memory, say) must not fail the pass: the float64 search needs no filter
    if (pcr_build_centroid_filter(ctx, t) != PCR_OK || (t->filter && !(t->filter_band > 0))) {
        fprintf(stderr, "[pcr] the float32 filter index of a voxel target could not be built (%s); its centroid searches stay in float64\n",
                pcr_last_error());
        (void)hipGetLastError();
        pcr_target_release(t->filter);
        t->filter = nullptr; t->filter_band = 0;
    }
}

// the deeper set of extended lists of a point target: built once the target has served PCR_HALO2_AFTER search + reduce
// passes (a failed build is not an error: the pass runs on the first set)
static void pass_lazy_deep_lists(pcr_context *ctx, pcr_target *t) {
    if (t->deep_tried || ++t->split_passes <= PCR_HALO2_AFTER) return;
    t->deep_tried = true;
    if (pcr_build_deep_lists(ctx, t) != PCR_OK) (void)hipGetLastError();
}

// use_filter: the searches of this pass go through the target's float32 filter index; deep: they may read the deeper lists
static void pass_fill_lin(Pass *ps, double max_dist, unsigned flags, bool use_filter, bool deep, int nblocks) {
    const pcr_context *ctx = ps->ctx;
    const pcr_target *t = ps->t;
    const pcr_scan *s = ps->s;
    LinArgs &a = ps->a;
    memset(&a, 0, sizeof a);
    a.sx = s->x; a.sy = s->y; a.sz = s->z; a.n = s->n;
    a.gf = t->gf; a.pts = t->pts; a.pn = t->pn;
    a.pts_last = (uint32_t)(t->is_voxel ? 0 : t->n + PCR_PTS_PAD - 1);
    a.gd = t->gd; a.means = t->means; a.vnorm = t->vnorm; a.vicov = t->vicov;
    a.cell_start = t->cell_start;
    if (use_filter) {
        a.gf = t->filter->gf; a.pts = t->filter->pts; a.cs_f = t->filter->cell_start;
        a.band_f = (float)(t->filter_band * 1.000001);
    }
    if (ps->q6) {
        // the filter is the target's own float32 index (a.gf / a.pts / cell_start as they are); the float64 side reads the
        // float64 coordinates in the same order through the voxel-target fields of the kernels
        a.gd = t->gq; a.means = t->pts64; a.cs_f = t->cell_start;
        a.band_f = (float)(t->band64 * 1.000001);
        flags |= PCR_IFLAG_NOGATE;
    }
    if (deep) {
        // (PCR_LIST_SET = 0 / 1 / 2, developer switch: every plain full search reads that set, near / mid / far, if the target has it)
        const char *fe = getenv("PCR_LIST_SET");
        const int force = fe && *fe ? atoi(fe) : -1;
        for (int k = 0, have = -1; k < PCR_DEEP_SETS; ++k) {      // a set the target lacks reads as the deepest one below it
            if (t->deep[k].cs) have = k;
            const int use = force < 0 ? have : (force >= 1 && force <= PCR_DEEP_SETS && t->deep[force - 1].cs ? force - 1 : -1);
            if (use < 0) continue;
            const pcr_target::ListSet &d = t->deep[use];
            a.deep[k].cs = d.cs; a.deep[k].pts = d.pts; a.deep[k].j = d.j; a.deep[k].lbox = d.lbox; a.deep[k].gbox = d.gbox; a.deep[k].halo = d.halo;
        }
        ps->list_force = force >= 1 && a.deep[0].halo > 0.f;
    }
    a.md_f = (float)max_dist; a.md_d = max_dist;
    const double bound = max_dist * (1.0 + 1e-6);
    a.bound2_f = (float)(bound * bound); a.bound2_d = bound * bound;
    set_filter_bound(a, bound);
    a.flags = flags;           // (public bits were masked by pass_setup: PCR_PUBLIC_FLAGS; internal bits are OR-ed in above)
    a.nblocks = nblocks;
    a.partials = ctx->d_partials;
    a.nn_j = s->nn_j; a.tile_ctr = ctx->d_tile_ctr + 9 * PCR_TICKET_STRIDE;
    a.pending = ctx->d_tile_ctr + 9 * PCR_TICKET_STRIDE + (size_t)PCR_TILE_CTRS * PCR_TILE_STRIDE;
    a.lb2 = s->lb2; a.umask = s->umask; a.ucnt = s->ucnt;
    a.mu_f = (float)(ctx->reuse_mu * cell_edge(t));
}

static void pass_fill_fin(Pass *ps) {
    const pcr_context *ctx = ps->ctx;
    const pcr_scan *s = ps->s;
    FinArgs &f = ps->f;
    memset(&f, 0, sizeof f);
    for (int i = 0; i < 3; ++i) { f.bb_c[i] = s->bb_c[i]; f.bb_e[i] = s->bb_e[i]; }
    f.local_len = ctx->local_frac * cell_edge(ps->t);
    f.deep_len = PCR_HALO2_MOVE * cell_edge(ps->t);
    f.far_len = PCR_HALO3_MOVE * cell_edge(ps->t);
    f.out_len = ps->t->heavy ? HUGE_VAL : PCR_HALO_OUT_MOVE * cell_edge(ps->t);      // (heavy targets: mid from deep_len on, as measured)
    if (ps->list_force) { f.deep_len = f.far_len = 0.0; f.out_len = HUGE_VAL; }       // (PCR_LIST_SET: whatever the step, the forced set)
    f.ucnt = s->ucnt; f.n_ucnt = ps->a.nblocks;
    f.partials = ctx->d_partials; f.tile_ctr = ctx->d_tile_ctr + 9 * PCR_TICKET_STRIDE; f.tickets = ctx->d_tile_ctr;
    f.nblocks = ps->a.nblocks; f.kind = ps->kind; f.out = ctx->d_out;
}

// (force_fused: a batched pass -- the fused kernel whatever the variant and the size of the scan)
static pcr_status pass_setup(Pass *ps, pcr_target *t, pcr_scan *s, int kind, double max_dist, unsigned flags, bool force_fused = false) {
    pcr_context *ctx = t->ctx;
    PCR_TRY(pass_validate(t, s, kind, max_dist));
    HIP_TRY(hipSetDevice(ctx->device));
    PCR_TRY(pcr_ensure_scratch(ctx, s->n));
    // one fused kernel or search + reduce?  variant 2 (default) decides by size: a small scan is latency-bound
    // and runs fused (tools/variant_crossover.py: 100 k points 74 vs 80 us per pass, 300 k 97 vs 92, 1.06 M 190 vs 151)
    // quirk Q6: always search + reduce, always a full search
    const bool q6 = pass_is_q6(t, kind);
    const bool one_kernel = (force_fused || pcr_pass_is_fused(ctx, s)) && !q6;
    pass_init(ps, t, s, kind, one_kernel, q6);
    // k_reduce streams: 4 blocks/CU
    const int nblocks_split = grid8(choose_blocks(ctx, s->n), ctx->num_cu * 4);
    PCR_TRY(pass_scan_buffers(ps, nblocks_split));
    // When the lazily built structures appear decides which kernels later passes run: the counters below move once per pass.
    const bool filter_ok = t->is_voxel && ctx->vox_filter && ctx->nn_mode != 3 && (!one_kernel || ctx->fuse_finalize);
    if (filter_ok) pass_lazy_filter(ctx, t, one_kernel);
    const bool deep_ok = !t->is_voxel && !one_kernel && !q6 && t->cs_h && nn_plain(ctx);
    if (deep_ok) pass_lazy_deep_lists(ctx, t);
    pass_fill_lin(ps, max_dist, flags & PCR_PUBLIC_FLAGS, filter_ok && t->filter, deep_ok, one_kernel ? choose_blocks(ctx, s->n) : nblocks_split);
    pass_fill_fin(ps);
    return PCR_OK;
}

static void pass_set_host_pose(Pass *ps, const double T[16]) {
    host_pose_k(T, &ps->a.hp);
    memcpy(ps->f.R, ps->a.hp.R, sizeof ps->f.R);
    ps->a.pose = nullptr; ps->f.pose = nullptr;
    if (ps->s->pose_valid) {
        PoseK q;
        host_pose_k(ps->s->prev_T, &q);
        memcpy(ps->a.hq.r32, q.r32, sizeof q.r32);
        memcpy(ps->a.hq.t32, q.t32, sizeof q.t32);
    }
}

// bound and margin of the float32 filter search (nn_point_filter) that go with a float64 search bound
static void set_filter_bound(LinArgs &a, double bound) {
    if (a.band_f <= 0.f) return;
    gn_filter_bounds((double)a.band_f, bound, &a.bound2_ff, &a.mu_ff);
}

// What the search of a pass does (gn_math.h: gn_choose_nn_mode) and the search bound that goes with it: a tracking
// search looks 5 % beyond the gate, so that a point with nothing in reach can be certified "still nothing" later.
static void pass_set_mode(Pass *ps, int mode) {
    ps->nn_mode = mode;
    ps->f.nn_mode = mode;
    const double md = ps->a.md_d;
    const double bound = mode == PCR_NN_FULL ? md * (1.0 + 1e-6) : md * 1.05;
    ps->a.bound2_f = (float)(bound * bound); ps->a.bound2_d = bound * bound;
    set_filter_bound(ps->a, bound);
}

static int host_choose_mode(const Pass *ps, const double T[16], double *motion_out) {
    const pcr_context *ctx = ps->ctx;
    const pcr_scan *s = ps->s;
    const pcr_target *t = ps->t;
    *motion_out = -1.0;
    const int have_prev = s->pose_valid && s->nn_serial == t->serial && s->nn_serial != 0;
    if (!have_prev) return PCR_NN_FULL;
    const double m = gn_typical_motion(s->prev_T, T, s->bb_c, s->bb_e);
    *motion_out = m;
    if (!ps->reuse_ready) return PCR_NN_FULL;
    return gn_choose_nn_mode(ctx->reuse, have_prev, s->track_valid ? 1 : 0, m, s->last_motion, ctx->reuse_tau * cell_edge(t));
}

// Which fused kernel a pass over this target runs -- the single launch and the batched one ask here, so the batch picks the
// instantiation a single fused launch would pick by construction
static FusedVariant fused_variant(const Pass *ps) {
    const pcr_target *t = ps->t;
    FusedVariant v;
    v.filt = t->is_voxel && ps->a.band_f > 0.f && ps->fused_fin;
    v.halo = t->is_voxel ? (v.filt && t->filter->cs_h != nullptr) : t->cs_h != nullptr;
    v.lb = t->is_voxel ? PCR_RANGE_PLAIN : (ps->a.gf.lbox != nullptr ? PCR_RANGE_BOXES : (ps->a.gf.xq > 0.f ? PCR_RANGE_XORDER : PCR_RANGE_PLAIN));
    v.gn = ps->gn_inline;
    return v;
}

// ---- pass_enqueue: the kernels of one pass onto the context's stream (no waiting) ----
static void enqueue_fused(Pass *ps, dim3 grid) {
    pcr_context *ctx = ps->ctx;
    ProfEvent ev;
    pcr_prof_begin(ctx, PCR_K_LINEARIZE, &ev);
    RoctxRange range("pcr:linearize");
    const FusedVariant v = fused_variant(ps);
#ifdef PCR_DEV
    if (!ps->fused_fin) pcr_dev_launch_linearize(ps->kind, v.halo, grid, ctx->stream, ps->a);
    else
#endif
    launch_fused(ps->kind, v, grid, ctx->stream, ps->a, ps->f);
    pcr_prof_end(ctx, &ev);
}

// grid of a search launch: exactly one resident generation of waves; they share the tiles dynamically
// (coop: the developer build's wave-cooperative kernel, which has an occupancy of its own)
struct SearchGrid { int64_t tiles, need; int nb; };     // tiles of the hand-out, the blocks they can keep busy, the blocks launched
static SearchGrid search_grid(const Pass *ps, bool filter, int mode, bool coop = false) {
    const pcr_context *ctx = ps->ctx;
    const bool vox = ps->t->is_voxel != 0;
    int64_t nb = (int64_t)ctx->num_cu * ctx->nn_blocks_per_cu[filter ? 3 : vox ? 1 : coop ? 2 : 0];
    if (!filter && !vox && mode == PCR_NN_FULL && !coop && ps->a.gf.lbox != nullptr) nb = (int64_t)ctx->num_cu * ctx->nn_blocks_lb;
    // tiles of the hand-out: 64 points per wave, or the 1024-point chunks of a LIST pass (one block per chunk)
    const int64_t tiles = mode == PCR_NN_LIST ? (ps->a.n + PCR_LIST_CHUNK - 1) / PCR_LIST_CHUNK : (ps->a.n + 63) / 64;
    const int64_t need = mode == PCR_NN_LIST ? tiles : (tiles + 3) / 4;
    return SearchGrid{tiles, need, grid8(nb < need ? nb : need)};
}

// the search without a float32 filter in front: a point target, or the centroids in float64 (through the row occupancy
// words where the gate spans enough rows of cells); mode and hand-out as ps says
static void launch_plain_search(const Pass *ps, dim3 nn_grid) {
    const pcr_context *ctx = ps->ctx;
    const pcr_target *t = ps->t;
    const LinArgs &a = ps->a;
    const int voxel = !t->is_voxel ? 0 : t->gd.rowocc != nullptr && (ctx->vox_occ >= 0 ? ctx->vox_occ != 0 : a.md_d / t->gd.h + 2.0 >= 5.0) ? 2 : 1;
    launch_nn_scan(voxel, ps->nn_mode, voxel == 0 && t->cs_h != nullptr, a.sched_local, nn_grid, ctx->stream, a);
}

// filter: the float32 filter search (voxel targets with a filter index, Q6)
static pcr_status enqueue_search(Pass *ps, dim3 grid, bool filter) {
    pcr_context *ctx = ps->ctx;
    const LinArgs &a = ps->a;
    const bool vox = ps->t->is_voxel != 0;
    const int mode = ps->nn_mode;
    ProfEvent ev;
    if (mode == PCR_NN_LIST) {
        // the previous matches that are provably still exact need no search (k_certify)
        pcr_prof_begin(ctx, PCR_K_CERTIFY, &ev);
        RoctxRange range("pcr:certify");
        launch_certify(vox, grid, ctx->stream, a);
        pcr_prof_end(ctx, &ev);
    }
    pcr_prof_begin(ctx, PCR_K_NN, &ev);
    {
        RoctxRange range("pcr:nn_search");
        const bool coop = !vox && !ps->q6 && ctx->nn_mode == 2;        // (developer build only: pcr_set_nn_mode)
        const SearchGrid g = search_grid(ps, filter, mode, coop);
        const int64_t tiles = g.tiles, nb = g.nb;
        const dim3 nn_grid((unsigned)nb);
        // hand-out policy: at most ~1.5 tiles per launched wave -> block-local (nn_tile_loop)
        // ... or the scan moved little since the previous pass: the far poses are where the cost of a tile varies 10x
        // and the global counters pay (1.06 M points, per pose: 235 / 185 / 108 / 55 / 52 us with the counters,
        // 221 / 203 / 111 / 51 / 40 block-local); the device-resident loop decides in k_gn_update (2)
        int local = tiles * 2 <= nb * 4 * 3 ? 1 : 0;
        // (only while a wave gets a handful of tiles: with 38 tiles per wave -- the 12.5 M-point shard -- the static
        // deal loses whatever the pose: plane_100m 2.93 vs 2.82 ms per pass, vplane_10m 1.075 vs 1.06)
        // Round 5: with the chunk interleave (an XCD's tiles spread over the whole scan) the block-local deal is balanced at the
        // far poses too and wins at EVERY pose of such scans (1.06 M points, search per trajectory: plane_b01 569 -> 531 us, icp_b01
        // 2316 -> 2282, resampled 928 -> 874; forced global counters 590 / 2541 / 966) -- but not with tens of tiles per wave
        // (vplane_10m 3492 -> 5174 us, plane_100m +12 %): profiles/r05_handout_policy.txt
        if (!local && mode != PCR_NN_LIST && tiles <= nb * 4 * 8) {
            if (PCR_TILE_INTERLEAVE) local = 1;
            else if (a.pose != nullptr) local = mode == PCR_NN_FULL ? 2 : 0;
            else if (ps->motion >= 0.0 && ps->motion < ps->f.local_len) local = 1;
        }
        if (ctx->tile_local >= 0) local = ctx->tile_local;
        ps->a.sched_local = local;
#ifdef PCR_DEV
        // (developer build, nn_mode 4: the MFMA-filtered search on every plain full search of a point target)
        const bool mfma = !vox && !ps->q6 && mode == PCR_NN_FULL && ps->t->n > 0 && ctx->nn_mode == 4;
        if (coop) {
            pcr_dev_launch_coop(nn_grid, ctx->stream, a);
        } else if (mfma) {
            const int64_t nbm = (int64_t)ctx->num_cu * ctx->nn_blocks_per_cu[4];
            launch_nn_mfma(ps->t->cs_h != nullptr, ps->a.sched_local == 1 ? 1 : 0, dim3((unsigned)grid8(nbm < g.need ? nbm : g.need)), ctx->stream, a);
        } else
#endif
        if (filter) {
            if (++ctx->filter_stamp == 0) {                    // (wrapped after 2^32 passes: start over)
                HIP_TRY(hipMemsetAsync(a.pending, 0, 4, ctx->stream));
                ctx->filter_stamp = 1;
            }
            ps->a.stamp = ctx->filter_stamp;
            const bool fhalo = ps->q6 ? ps->t->cs_h != nullptr : ps->t->filter->cs_h != nullptr;
            launch_nn_filter(fhalo, ps->a.sched_local == 1 ? 1 : 0, !ps->fused_fin, ps->q6, nn_grid, ctx->stream, a);
        } else {
            // host-driven pass over a point target: the list set by how far the scan moved since the previous pass (unknown: the deepest one)
            if (!vox && a.pose == nullptr && mode == PCR_NN_FULL) {
                const double m = ps->motion;
                const int k = m < 0.0 ? 1 : (m >= ps->f.out_len ? -1 : (m >= ps->f.far_len ? 1 : (m >= ps->f.deep_len ? 0 : -1)));
                if (k >= 0 && a.deep[k].halo > 0.f) use_lists(ps->a.gf, a.deep[k]);
            }
            launch_plain_search(ps, nn_grid);
        }
        ps->s->nn_serial = ps->t->serial;      // nn_j now holds matches against this target
    }
    pcr_prof_end(ctx, &ev);
    return PCR_OK;
}

// (filter: the pending points of the filter search are settled in the prologue of the reduce kernel)
static void enqueue_reduce(Pass *ps, dim3 grid, bool filter) {
    pcr_context *ctx = ps->ctx;
    ProfEvent ev;
    pcr_prof_begin(ctx, PCR_K_REDUCE, &ev);
    RoctxRange range("pcr:reduce");
#ifdef PCR_DEV
    if (!ps->fused_fin) pcr_dev_launch_reduce(ps->kind, grid, ctx->stream, ps->a);
    else
#endif
    launch_reduce_kind(ps->kind, filter, grid, ctx->stream, ps->a, ps->f);
    pcr_prof_end(ctx, &ev);
}

static pcr_status pass_enqueue(Pass *ps) {
    pcr_context *ctx = ps->ctx;
#ifdef PCR_DEV
    {   // developer timing experiments on the pending-point prologue (results are WRONG when set)
        static const int dbg = getenv("PCR_FIX_DEBUG") ? atoi(getenv("PCR_FIX_DEBUG")) : 0;
        if (dbg) ps->a.flags |= (unsigned)(dbg & 3) << 28;
    }
#endif
    const dim3 grid(ps->a.nblocks);
    if (ctx->prof_on) ctx->prof_this_pass = (ctx->prof_pass++ % (uint64_t)ctx->prof_period) == 0;
    if (ps->one_kernel) {
        enqueue_fused(ps, grid);
    } else {
        const bool filter = (ps->t->is_voxel && ps->nn_mode == PCR_NN_FULL && ps->a.band_f > 0.f) || ps->q6;
        PCR_TRY(enqueue_search(ps, grid, filter));
        enqueue_reduce(ps, grid, filter);
    }
    HIP_TRY(hipGetLastError());
#ifdef PCR_DEV
    if (!ps->fused_fin) {
        ProfEvent ev;
        pcr_prof_begin(ctx, PCR_K_FINALIZE, &ev);
        pcr_dev_launch_finalize(ctx->stream, ps->f);
        pcr_prof_end(ctx, &ev);
        HIP_TRY(hipGetLastError());
    }
#endif
    return PCR_OK;
}

// Spin on a word in pinned host memory that a kernel writes, then fall back to a blocking wait.
template <typename Pred>
static pcr_status wait_host_word(pcr_context *ctx, Pred ready, const char *what) {
    for (long spin = 0; spin < 4000000L; ++spin) {
        if (ready()) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return PCR_OK; }
        __builtin_ia32_pause();
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));     // very long pass (or a fault): block, then re-check
    if (!ready()) { pcr_set_error("%s did not report completion", what); return PCR_ERR_HIP; }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return PCR_OK;
}

// Rare 6-60 ms stalls of ONE call early in a process ("12-42 ms, about once per 1500 passes") were
// root-caused in round 3 (tools/stall_study.py, PCR_STALL_DEBUG=1; profiles/archive/r03_stall_root_cause.txt): the calling
// thread is DESCHEDULED -- on a CPU for 0.03-0.08 ms of a 41 ms stall -- while the container's cgroup reports one
// more throttled period (cpu.max = 16 CPUs per 100 ms on the GPU box): the thread pools of the host libraries
// (256 visible CPUs) burn the CPU quota during start-up and the kernel parks every thread of the cgroup until the
// next period.  Durations are 6.6 ms + k x 10 ms (scheduler ticks); the stall lands in the enqueue or in the spin,
// wherever the thread happens to be.  Neither the GPU nor the HIP runtime is involved: with the host thread pools
// capped (OMP_NUM_THREADS / OPENBLAS_NUM_THREADS) 25 of 25 fresh processes and 1e6 consecutive passes stay below
// 1 ms.  The hipStreamQuery cadence of round 2 rested on a wrong theory (20 of 25 processes stalled with it, 23 of
// 25 without); it is kept only as an opt-in knob (PCR_RETIRE_PERIOD, default off).
static void retire_completed(pcr_context *ctx) {
    if (ctx->retire_period > 0 && ++ctx->passes_since_query >= (uint32_t)ctx->retire_period) {
        ctx->passes_since_query = 0;
        (void)hipStreamQuery(ctx->stream);
    }
}

pcr_status pcr_run_linearize(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist,
                             unsigned flags, double out[29]) {
    Pass ps;
    PCR_TRY(pass_setup(&ps, t, s, kind, max_dist, flags));
    pcr_context *ctx = ps.ctx;
    pass_set_host_pose(&ps, T);
    double motion = -1.0;
    const int mode = ps.one_kernel ? PCR_NN_FULL : host_choose_mode(&ps, T, &motion);
    ps.motion = motion;
    pass_set_mode(&ps, mode);
    const bool use_comm = ctx->comm != nullptr && !(flags & PCR_FLAG_LOCAL_ONLY);
    // single GPU: the finalize step writes the result and a sequence number straight into pinned host
    // memory (no copy command, no stream query); with a communicator the all-reduce sits in between
    const bool direct = !use_comm && ctx->h_out_dev != nullptr;
    volatile uint32_t *flag = (volatile uint32_t *)(ctx->h_out + 32);
    ps.f.host_out = direct ? ctx->h_out_dev : nullptr;
    ps.f.host_flag = direct ? (volatile uint32_t *)(ctx->h_out_dev + 32) : nullptr;
    if (++ctx->seq == 0) ctx->seq = 1;      // (never 0: the sequence words start out zeroed)
    const uint32_t seq = ctx->seq;
    ps.f.seq = seq;
    // host fold: the 8 group leaders of the in-kernel fold store their rows to pinned memory and the host adds them -- no
    // second ticket level on the device (ticket_fold_emit).  Not for ICP (the emitting block forms H from the sums with
    // multiplications, which host and device need not contract alike) and not for a LIST pass (its count of searched points
    // is summed by the emitting block); d_out is not written by such a pass, and nothing reads it after a direct one.
    const bool host_fold = direct && ctx->host_fold && ctx->h_rows_dev != nullptr && ps.fused_fin && kind != PCR_ICP && mode != PCR_NN_LIST;
    volatile uint32_t *gflags = (volatile uint32_t *)(ctx->h_rows + 8 * 32);
    if (host_fold) {
        ps.f.host_rows = ctx->h_rows_dev;
        ps.f.host_gflags = (volatile uint32_t *)(ctx->h_rows_dev + 8 * 32);
        ctx->host_fold_passes += 1;
    }
    const bool stall_dbg = ctx->stall_debug;
    struct timespec ts0, ts1, ts2, tc0, tc2;
    if (stall_dbg) { clock_gettime(CLOCK_MONOTONIC, &ts0); clock_gettime(CLOCK_THREAD_CPUTIME_ID, &tc0); }
    PCR_TRY(pass_enqueue(&ps));
    if (stall_dbg) clock_gettime(CLOCK_MONOTONIC, &ts1);
    // what this pass leaves behind for the next one over the same scan
    memcpy(s->prev_T, T, sizeof s->prev_T);
    s->pose_valid = !ps.one_kernel;
    s->track_valid = mode != PCR_NN_FULL;
    s->last_mode = mode; s->last_motion = motion; s->last_marked = mode == PCR_NN_LIST ? -1 : 0;
    s->st_passes[mode] += 1;

    bool flagged = direct;
    if (use_comm) {
        ProfEvent ev;
        pcr_prof_begin(ctx, PCR_K_ALLREDUCE, &ev);
        RoctxRange range("pcr:allreduce29");
        pcr_status cs = pcr_comm_allreduce29(ctx, ctx->d_out);
        if (cs == PCR_OK && ctx->h_out_dev) {
            launch_publish(ctx->stream, ctx->d_out, ctx->h_out_dev, (volatile uint32_t *)(ctx->h_out_dev + 32), seq);
            flagged = true;
        }
        pcr_prof_end(ctx, &ev);
        if (cs != PCR_OK) return cs;
        HIP_TRY(hipGetLastError());
    }
    if (host_fold) {
        auto all_groups = [&] {
            for (int g = 0; g < 8; ++g)
                if (gflags[g * PCR_GFLAG_STRIDE] != seq) return false;
            return true;
        };
        PCR_TRY(wait_host_word(ctx, all_groups, "the fold of a group"));
        gn_fold8_rows(ctx->h_rows, ctx->h_out, 29);
    } else if (flagged) {
        PCR_TRY(wait_host_word(ctx, [&] { return *flag == seq; }, "finalize kernel"));
    } else {
        HIP_TRY(hipMemcpyAsync(ctx->h_out, ctx->d_out, sizeof(double) * 31, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    // the result is in h_out, whichever way it got there
    if (use_comm && pcr_comm_failed_now(ctx)) {
        pcr_set_error("peer-to-peer exchange: a peer did not arrive (its sums were not reduced)");
        return PCR_ERR_COMM;
    }
    if (stall_dbg && flagged) {              // developer (PCR_STALL_DEBUG): where did a slow call spend its time?
        clock_gettime(CLOCK_MONOTONIC, &ts2); clock_gettime(CLOCK_THREAD_CPUTIME_ID, &tc2);
        const double cpu = (tc2.tv_sec - tc0.tv_sec) * 1e3 + (tc2.tv_nsec - tc0.tv_nsec) * 1e-6;
        const double enq = (ts1.tv_sec - ts0.tv_sec) * 1e3 + (ts1.tv_nsec - ts0.tv_nsec) * 1e-6;
        const double wait = (ts2.tv_sec - ts1.tv_sec) * 1e3 + (ts2.tv_nsec - ts1.tv_nsec) * 1e-6;
        if (enq + wait > 1.0) {
            fprintf(stderr, "[pcr stall] seq %u: enqueue %.3f ms, wait for the result %.3f ms; this thread was ON a CPU for %.3f ms of it\n",
                    seq, enq, wait, cpu);
        }
    }
    for (int i = 0; i < 29; ++i) out[i] = ctx->h_out[i];
    if (mode == PCR_NN_LIST && !use_comm) {      // (the count of one rank says nothing about the all-reduced sums)
        s->last_marked = (int64_t)ctx->h_out[29];
        s->st_marked += s->last_marked; s->st_listed_of += s->n;
    }
    if (flagged) retire_completed(ctx);
    return PCR_OK;
}

// ---- the host side of the device-resident loop (pcr_run_align, pcr_run_batch) ----
// Keep the queue AHEAD iterations beyond the slowest unfinished item and never wait on the stream.  progress(&fin) returns how
// many items are still running and sets fin to the fewest passes any of them has completed; enqueue() puts one iteration on
// the stream; *enq counts them (the caller may go on counting).  After 4 000 000 idle spins -- a very long pass, or a fault --
// block once, look again, and fail if nothing moved.
static const int AHEAD = 2;
template <typename Progress, typename Enqueue>
static pcr_status drive_device_loop(pcr_context *ctx, int max_iter, int *enq, Progress &&progress, Enqueue &&enqueue, const char *stuck) {
    long spin = 0;
    for (;;) {
        int fin = 0;
        if (progress(&fin) == 0) return PCR_OK;
        if (*enq < max_iter && *enq < fin + AHEAD) {
            PCR_TRY(enqueue());
            ++*enq;
            spin = 0;
            continue;
        }
        __builtin_ia32_pause();
        if (++spin > 4000000L) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            int fin2 = 0;
            if (progress(&fin2) != 0 && fin2 == fin && !(*enq < max_iter)) {
                pcr_set_error("%s", stuck);
                return PCR_ERR_HIP;
            }
            spin = 0;
        }
    }
}

// ---- Registration.align behind the boundary, device-resident (registration.py:71-113) -------------
// The pose lives in HBM; every iteration is k_nn_scan + k_reduce_finalize + k_gn_update (one wave:
// dx = -solve(H, g), the |dx| < tol test and T <- plus(T, dx)).  The host only keeps the
// queue a couple of iterations ahead of the GPU and watches two words in pinned memory: no host round
// trip, no device-to-host copy and no host solve between iterations.  Launches that arrive after
// convergence see pose->done and return at once.  With a communicator the 29 sums are all-reduced
// between the fold and the step (k_gn_update); every rank issues the same number of collectives (see below).
pcr_status pcr_run_align(pcr_target *t, pcr_scan *s, int kind, const double T_init[16], int max_iter, double tol,
                         double max_dist, unsigned flags, double T_out[16], int *iterations, double *trace_or_null) {
    Pass ps;
    PCR_TRY(pass_setup(&ps, t, s, kind, max_dist, flags));
    pcr_context *ctx = ps.ctx;
    if (max_iter <= 0) {
        memcpy(T_out, T_init, 16 * sizeof(double));
        if (iterations) *iterations = 0;
        return PCR_OK;
    }
    s->pose_valid = false; s->track_valid = false;       // (the loop's own bookkeeping lives in PoseDev)
    if (ctx->trace_cap < max_iter) {
        if (ctx->d_trace) HIP_TRY(hipFree(ctx->d_trace));
        ctx->d_trace = nullptr; ctx->trace_cap = 0;
        HIP_TRY(pcr_malloc_retry((void **)&ctx->d_trace, sizeof(double) * 45 * (size_t)max_iter));
        ctx->trace_cap = max_iter;
    }
    const bool use_comm = ctx->comm != nullptr && !(flags & PCR_FLAG_LOCAL_ONLY);
    volatile unsigned long long *state = (volatile unsigned long long *)(ctx->h_out + 56);
    *state = 0;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    ps.a.pose = ctx->d_pose;
    FinArgs &f = ps.f;
    f.pose = ctx->d_pose; f.max_iter = max_iter; f.tol = tol;
    f.trace = ctx->d_trace;
    f.host_T = ctx->h_out_dev + 40;
    f.host_state = (volatile unsigned long long *)(ctx->h_out_dev + 56);
    launch_pose_init(ctx->stream, ctx->d_pose, T_init, max_iter);
    HIP_TRY(hipGetLastError());

    auto passes_done = [&] { return (int)(unsigned)(*state & 0xffffffffull); };
    auto loop_done = [&] { return (int)(unsigned)(*state >> 32); };
    // One iteration = the pass, (multi-GPU) the in-stream all-reduce of its 29 sums, the one-wave update.  The host
    // keeps the queue AHEAD iterations beyond the one the GPU reports and never waits on the stream.
    // Multi-GPU: every rank must issue the SAME number of collectives, but each reads the (identical, all-reduced)
    // state word at its own time.  A rank enqueues iteration e only while e < passes_done + AHEAD, so when it sees
    // the loop end after `it` passes it has enqueued at most min(max_iter, it + AHEAD) iterations -- a number every
    // rank can compute; each tops its queue up to exactly that (launches behind the end are no-ops, their
    // all-reduces move stale sums): no host synchronisation between iterations, at most AHEAD dead all-reduces.
    int enq = 0;
    ps.gn_inline = ps.one_kernel && ps.fused_fin && !use_comm;
    auto enqueue_iteration = [&]() -> pcr_status {
        retire_completed(ctx);
        PCR_TRY(pass_enqueue(&ps));
        if (use_comm) {
            ProfEvent ev;
            pcr_prof_begin(ctx, PCR_K_ALLREDUCE, &ev);
            pcr_status cs = pcr_comm_allreduce29(ctx, ctx->d_out, ctx->d_pose);
            pcr_prof_end(ctx, &ev);
            if (cs != PCR_OK) return cs;
        }
        if (!ps.gn_inline) launch_gn_update(ctx->stream, f);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    };
    PCR_TRY(drive_device_loop(ctx, max_iter, &enq, [&](int *fin) {
        const unsigned long long w = *state;           // (one 8-byte word: done and passes belong together)
        *fin = (int)(unsigned)(w & 0xffffffffull);
        return (int)(unsigned)(w >> 32) == PCR_LOOP_RUNNING ? 1 : 0;
    }, enqueue_iteration, "device Gauss-Newton loop made no progress"));
    if (use_comm && loop_done() == PCR_LOOP_COMMFAIL) {
        //  this rank's exchange timed out: no top-up -- the peers are gone or late, and whatever they do with
        // their own timeouts, this call must not report a pose
        (void)hipStreamSynchronize(ctx->stream);
        pcr_set_error("peer-to-peer exchange: a peer did not arrive after %d iteration(s)", passes_done());
        return PCR_ERR_COMM;
    }
    if (use_comm) {
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const int it_end = passes_done();
        const int target = it_end + AHEAD < max_iter ? it_end + AHEAD : max_iter;
        for (; enq < target; ++enq) PCR_TRY(enqueue_iteration());
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const int done = loop_done(), it = passes_done();
    if (!t->is_voxel && !ps.one_kernel) t->split_passes += it > 1 ? it - 1 : 0;     // (pass_setup counted one)
    for (int i = 0; i < 16; ++i) T_out[i] = ctx->h_out[40 + i];
    if (iterations) *iterations = it;
    if (trace_or_null && it > 0) {
        HIP_TRY(hipMemcpyAsync(trace_or_null, ctx->d_trace, sizeof(double) * 45 * (size_t)it, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (use_comm && pcr_comm_failed_now(ctx)) {
        pcr_set_error("peer-to-peer exchange: a peer did not arrive");
        return PCR_ERR_COMM;
    }
    if (done == PCR_LOOP_SINGULAR) {
        pcr_set_error("Singular matrix");
        return PCR_ERR_SINGULAR;
    }
    return PCR_OK;
}

// ---- batched passes: many scans / start poses against one target in one launch (pcr_linearize_batch, pcr_align_batch) ----
static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The loop is pcr_run_align's (drive_device_loop): one launch per iteration for the WHOLE batch, queued AHEAD iterations beyond the slowest
// unfinished item; every item reports (done << 32 | passes) in its own pinned word and its final pose next to it; an item
// that is done makes its blocks of the later launches return at load_pose.  No stream synchronisation between iterations.
pcr_status pcr_run_batch(pcr_target *t, pcr_scan *const *scans, int n_items, int kind, const double *T, bool align, int max_iter,
                         double tol, double max_dist, unsigned flags, double *out29, double *T_out, int *iterations,
                         pcr_status *item_status, double *trace_or_null) {
    pcr_context *ctx = t->ctx;
    PCR_TRY(refuse_comm_and_q6(t, kind, "batched passes", "batched PlaneICP passes", "quirk Q6 runs search + reduce"));
    PCR_REQUIRE(n_items >= 0 && n_items <= 65535, "a batch call takes at most 65535 items");
    if (n_items == 0) return PCR_OK;
    pcr_scan *big = scans[0];
    for (int i = 1; i < n_items; ++i) if (scans[i]->n > big->n) big = scans[i];
    Pass ps;
    // (pass_setup also makes sure the context's pass scratch exists -- pcr_ensure_scratch: a one-time, size-independent
    // allocation that fixes ctx->max_blocks, which choose_blocks reads; the batch itself uses none of those buffers but d_tile_ctr)
    PCR_TRY(pass_setup(&ps, t, big, kind, max_dist, flags, true));
    if (!ps.one_kernel || !ps.fused_fin) {
        pcr_set_error("batched passes need the fused pipeline (pcr_set_fuse_finalize(1))");
        return PCR_ERR_UNSUPPORTED;
    }
    const size_t B = (size_t)n_items;
    if (align && max_iter <= 0) {                      // as pcr_run_align: nothing runs
        memcpy(T_out, T, B * 16 * sizeof(double));
        for (size_t i = 0; i < B; ++i) { if (iterations) iterations[i] = 0; if (item_status) item_status[i] = PCR_OK; }
        return PCR_OK;
    }
    // ---- device block: descriptors | tickets | poses | sums | partial rows | trace rows (from / back to the context's cache)
    std::vector<int> nb(B);
    size_t rows = 0;
    int max_nb = 0;
    for (size_t i = 0; i < B; ++i) {
        nb[i] = choose_blocks(ctx, scans[i]->n);
        rows += (size_t)nb[i] + 8;
        if (nb[i] > max_nb) max_nb = nb[i];
    }
    const size_t trace_rows = align && trace_or_null ? (size_t)max_iter : 0;
    const size_t pose_stride = round_up(sizeof(PoseDev), 128), ticket_bytes = sizeof(uint32_t) * 9 * PCR_TICKET_STRIDE;
    const size_t off_tickets = round_up(B * sizeof(BatchItem), 256);      // (the descriptors sit at the start of the block)
    const size_t off_pose = off_tickets + B * ticket_bytes;
    const size_t off_out = off_pose + B * pose_stride;
    const size_t off_part = off_out + B * 32 * sizeof(double);
    const size_t off_trace = off_part + rows * 32 * sizeof(double);
    const size_t total = off_trace + B * trace_rows * 45 * sizeof(double);
    // The block goes back to the cache when this function returns, while up to AHEAD trailing launches that read `items` and
    // the items' PoseDev may still be queued: safe because every user of the cache runs on the context's ONE stream, behind them.
    DevBuf<char> ws;
    HIP_TRY(ws.alloc_bytes(total));
    // ---- pinned block: per item 24 doubles (pose 16, state word, padding) | 32 sums per item | staging of the descriptors
    const size_t h_state = 0, h_out = h_state + B * 24 * sizeof(double), h_items = h_out + B * 32 * sizeof(double);
    const size_t h_need = h_items + B * sizeof(BatchItem);
    if (ctx->h_batch_cap < h_need) {
        if (ctx->h_batch) { HIP_TRY(hipStreamSynchronize(ctx->stream)); HIP_TRY(hipHostFree(ctx->h_batch)); }
        ctx->h_batch = nullptr; ctx->h_batch_dev = nullptr; ctx->h_batch_cap = 0;
        const size_t cap = round_up(h_need * 2 > 65536 ? h_need * 2 : 65536, 4096);
        HIP_TRY(hipHostMalloc((void **)&ctx->h_batch, cap, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&ctx->h_batch_dev, ctx->h_batch, 0));
        ctx->h_batch_cap = cap;
    }
    BatchItem *hi = (BatchItem *)(ctx->h_batch + h_items);
    auto state_word = [&](size_t i) { return (volatile unsigned long long *)(ctx->h_batch + h_state + (i * 24 + 16) * sizeof(double)); };
    auto host_pose = [&](size_t i) { return (const double *)(ctx->h_batch + h_state + i * 24 * sizeof(double)); };
    size_t row = 0;
    for (size_t i = 0; i < B; ++i) {
        const pcr_scan *s = scans[i];
        BatchItem &d = hi[i];
        memset(&d, 0, sizeof d);
        d.sx = s->x; d.sy = s->y; d.sz = s->z; d.n = s->n;
        d.partials = (double *)(ws.p + off_part) + row * 32;
        row += (size_t)nb[i] + 8;
        d.tickets = (uint32_t *)(ws.p + off_tickets + i * ticket_bytes);
        d.pose = align ? (PoseDev *)(ws.p + off_pose + i * pose_stride) : nullptr;
        d.out = (double *)(ws.p + off_out) + i * 32;
        d.trace = trace_rows ? (double *)(ws.p + off_trace) + i * trace_rows * 45 : nullptr;
        d.host_T = (double *)(ctx->h_batch_dev + h_state + i * 24 * sizeof(double));
        d.host_state = (unsigned long long *)(ctx->h_batch_dev + h_state + (i * 24 + 16) * sizeof(double));
        d.nblocks = nb[i];
        for (int k = 0; k < 3; ++k) { d.bb_c[k] = s->bb_c[k]; d.bb_e[k] = s->bb_e[k]; }
        memcpy(d.T, T + 16 * i, sizeof d.T);
        *state_word(i) = 0;
    }
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    const BatchItem *items = (const BatchItem *)ws.p;
    HIP_TRY(hipMemcpyAsync(ws.p, hi, B * sizeof(BatchItem), hipMemcpyHostToDevice, ctx->stream));
    launch_batch_init(ctx->stream, items, (unsigned)B, align ? max_iter : 0);
    HIP_TRY(hipGetLastError());

    ps.a.pose = nullptr; ps.f.pose = nullptr;          // (per item: the descriptor's)
    // (ps.f.tile_ctr stays the context's: every item's emitting block re-zeroes those counters in finalize_emit -- all writers
    // store 0 and the fused kernels never read them, so the concurrent stores are harmless)
    ps.f.max_iter = max_iter; ps.f.tol = tol;
    ps.gn_inline = align;                              // (GN = the device-resident loop)
    const FusedVariant variant = fused_variant(&ps);
    const dim3 grid((unsigned)max_nb, (unsigned)B);
    auto enqueue_pass = [&]() -> pcr_status {
        retire_completed(ctx);
        ProfEvent ev;
        if (ctx->prof_on) ctx->prof_this_pass = (ctx->prof_pass++ % (uint64_t)ctx->prof_period) == 0;
        pcr_prof_begin(ctx, PCR_K_LINEARIZE, &ev);
        {
            RoctxRange range("pcr:linearize_batch");
            launch_fused_batch(kind, variant, grid, ctx->stream, ps.a, ps.f, items);
        }
        pcr_prof_end(ctx, &ev);
        HIP_TRY(hipGetLastError());
        return PCR_OK;
    };

    if (!align) {
        PCR_TRY(enqueue_pass());
        double *ho = (double *)(ctx->h_batch + h_out);
        HIP_TRY(hipMemcpyAsync(ho, ws.p + off_out, B * 32 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < B; ++i) memcpy(out29 + 29 * i, ho + 32 * i, 29 * sizeof(double));
        return PCR_OK;
    }

    // what the unfinished items report: how many there are and the fewest passes any of them has completed
    auto progress = [&](int *fin) {
        int running = 0, lo = 0x7fffffff;
        for (size_t i = 0; i < B; ++i) {
            const unsigned long long w = *state_word(i);
            if ((int)(unsigned)(w >> 32) != PCR_LOOP_RUNNING) continue;
            ++running;
            const int p = (int)(unsigned)(w & 0xffffffffull);
            if (p < lo) lo = p;
        }
        *fin = lo;
        return running;
    };
    int enq = 0;
    PCR_TRY(drive_device_loop(ctx, max_iter, &enq, progress, enqueue_pass, "device Gauss-Newton loop of a batch made no progress"));
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    for (size_t i = 0; i < B; ++i) {
        const unsigned long long w = *state_word(i);
        const double *hT = host_pose(i);
        for (int k = 0; k < 16; ++k) T_out[16 * i + k] = hT[k];
        if (iterations) iterations[i] = (int)(unsigned)(w & 0xffffffffull);
        if (item_status) item_status[i] = (int)(unsigned)(w >> 32) == PCR_LOOP_SINGULAR ? PCR_ERR_SINGULAR : PCR_OK;
    }
    if (trace_rows) {
        HIP_TRY(hipMemcpyAsync(trace_or_null, ws.p + off_trace, B * trace_rows * 45 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return PCR_OK;
}

// ---- rows passes: the search half of a search + reduce pass, then k_rows where the reduce kernel would go (rows.hip) ----
// The search is an ordinary FULL search (variant 1 whatever the scan size: the fused small-scan kernel keeps its matches in
// registers) into a match buffer of THIS call, so the scan's own nn_j / lb2 / umask and its reuse state (track_valid,
// pose_valid, nn_serial) stay exactly as the previous pass left them, and none of the target's lazily built structures is
// built or counted here: a following pcr_linearize / pcr_align runs the kernels, and returns the bits, it would have without
// the rows call.  Tiles are dealt block-locally (nn_tile_loop<1>): the global tile counters are re-armed by the reduce
// kernel's fold, which does not run here.  Voxel targets are searched in float64 (no float32 filter, hence no pending
// points): the filter is exact by construction, so the matches are the ones pcr_linearize finds.
// NOT measured: the block-local deal at EVERY scan size.  pass_enqueue records it as the loser once a wave gets tens of
// tiles (scans of ~10 M points and more); such a rows pass is correct but its search is slower than pcr_linearize's.
static pcr_status rows_search(Pass *ps, DevBuf<uint32_t> *nn, pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist,
                              unsigned flags, bool caller_order = true) {
    PCR_TRY(pass_validate(t, s, kind, max_dist));
    pcr_context *ctx = t->ctx;
    PCR_TRY(refuse_comm_and_q6(t, kind, "rows passes", "PlaneICP rows", "quirk Q6"));
    PCR_REQUIRE(!caller_order || !s->sorted || s->order != nullptr, "a Morton-sorted scan needs PCR_FLAG_KEEP_ORDER (or PCR_FLAG_NO_SCAN_SORT) for rows in the caller's order");
    HIP_TRY(hipSetDevice(ctx->device));
    PCR_TRY(pcr_ensure_scratch(ctx, s->n));
    pass_init(ps, t, s, kind, false, false);
    HIP_TRY(nn->alloc((size_t)(s->n > 0 ? s->n : 1)));
    pass_fill_lin(ps, max_dist, flags & PCR_PUBLIC_FLAGS, false, false, 8);
    LinArgs &a = ps->a;
    a.nn_j = nn->p; a.lb2 = nullptr; a.umask = nullptr; a.ucnt = nullptr;
    host_pose_k(T, &a.hp);
    pass_set_mode(ps, PCR_NN_FULL);
    a.sched_local = 1;
    if (s->n == 0) return PCR_OK;
    RoctxRange range("pcr:rows_search");
    launch_plain_search(ps, dim3((unsigned)search_grid(ps, false, PCR_NN_FULL).nb));
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}

// the same for a kernel of another translation unit (gicp.hip, which reads the scan in device order: caller_order = false)
pcr_status pcr_rows_search(LinArgs *a, DevBuf<uint32_t> *nn, pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist,
                           unsigned flags, bool caller_order) {
    Pass ps;
    PCR_TRY(rows_search(&ps, nn, t, s, kind, T, max_dist, flags, caller_order));
    *a = ps.a;
    return PCR_OK;
}

// the streaming grid of k_rows: as many blocks as choose_blocks wants, not rounded to 8 (no per-XCD spans, no fold)
static dim3 rows_grid(const pcr_context *ctx, int64_t n) {
    const int64_t nb = blocks_wanted(ctx, n);
    return dim3((unsigned)(nb < 1 ? 1 : nb));
}

pcr_status pcr_run_rows(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags, double *J,
                        double *r, double *w, double *W_or_null, int64_t *idx_or_null) {
    Pass ps;
    DevBuf<uint32_t> nn;
    PCR_TRY(rows_search(&ps, &nn, t, s, kind, T, max_dist, flags));
    pcr_context *ctx = ps.ctx;
    const int64_t n = s->n;
    if (n == 0) return PCR_OK;
    const size_t m = (kind == PCR_PLANE || kind == PCR_VPLANE) ? 1 : 3;
    const bool want_W = kind == PCR_NDT && W_or_null != nullptr;
    DevBuf<double> d_J, d_r, d_w, d_W;
    DevBuf<int64_t> d_idx;
    HIP_TRY(d_J.alloc((size_t)n * m * 6)); HIP_TRY(d_r.alloc((size_t)n * m)); HIP_TRY(d_w.alloc((size_t)n));
    if (want_W) HIP_TRY(d_W.alloc((size_t)n * 9));
    if (idx_or_null) HIP_TRY(d_idx.alloc((size_t)n));
    RowArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.order = s->order; ra.J = d_J.p; ra.r = d_r.p; ra.w = d_w.p; ra.W = d_W.p; ra.idx = d_idx.p;
    {
        RoctxRange range("pcr:rows");
        launch_rows(kind, 0, rows_grid(ctx, n), ctx->stream, ps.a, ra);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(J, d_J.p, 8 * (size_t)n * m * 6, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(r, d_r.p, 8 * (size_t)n * m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(w, d_w.p, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (want_W) HIP_TRY(hipMemcpyAsync(W_or_null, d_W.p, 8 * (size_t)n * 9, hipMemcpyDeviceToHost, ctx->stream));
    if (idx_or_null) HIP_TRY(hipMemcpyAsync(idx_or_null, d_idx.p, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PCR_OK;
}

pcr_status pcr_run_terms(pcr_target *t, pcr_scan *s, int kind, const double T[16], double max_dist, unsigned flags,
                         DevBuf<double> *P, int64_t *stride, DevBuf<int64_t> *col_idx, int64_t *n_in) {
    Pass ps;
    DevBuf<uint32_t> nn;
    PCR_TRY(rows_search(&ps, &nn, t, s, kind, T, max_dist, flags));
    pcr_context *ctx = ps.ctx;
    const int64_t n = s->n;
    *n_in = 0; *stride = n > 0 ? n : 1;
    if (n == 0) return PCR_OK;
    DevBuf<uint32_t> d_flag, d_off, d_inv;
    HIP_TRY(d_flag.alloc((size_t)n + 1)); HIP_TRY(d_off.alloc((size_t)n + 1));
    if (s->order) HIP_TRY(d_inv.alloc((size_t)n));
    HIP_TRY(hipMemsetAsync(d_flag.p + n, 0, sizeof(uint32_t), ctx->stream));
    RowArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.order = s->order; ra.flag = d_flag.p; ra.inv = d_inv.p;
    RoctxRange range("pcr:terms");
    launch_rows(kind, 2, rows_grid(ctx, n), ctx->stream, ps.a, ra);
    HIP_TRY(hipGetLastError());
    PCR_TRY(pcr_rows_offsets(ctx, d_flag.p, d_off.p, n + 1));
    // the column stride is the scan size, so the terms kernel does not wait for the count to cross PCIe.  The price is memory:
    // P is 28 x n doubles whatever the gated-in count (224 bytes per SCAN point: 237 MB at 1.06 M points, 2.2 GB at 10 M), and
    // it, the flags, offsets, inverse permutation, column indices and the match buffer (another 24 bytes per point) are
    // allocated by every call -- from the context's block cache after the first one (include/pcr.h says so to callers)
    HIP_TRY(P->alloc((size_t)28 * (size_t)n)); HIP_TRY(col_idx->alloc((size_t)n));
    ra.off = d_off.p; ra.P = P->p; ra.stride = n; ra.col_idx = col_idx->p;
    launch_rows(kind, 1, rows_grid(ctx, n), ctx->stream, ps.a, ra);
    HIP_TRY(hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off.p + n, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_in = (int64_t)total;
    return PCR_OK;
}

pcr_status pcr_run_nn(pcr_target *t, const float *d_q, int64_t m, double r_max, void *d_dist, int64_t *d_idx, int f64) {
    pcr_context *ctx = t->ctx;
    if (m == 0) return PCR_OK;
    const bool bounded = r_max > 0 && r_max < 1e300 * 1e300;
    const double inf = __builtin_inf(), rmax = bounded ? r_max : inf;
    ProfEvent ev;
    ctx->prof_this_pass = ctx->prof_on;            // (pass sampling applies to passes only)
    pcr_prof_begin(ctx, PCR_K_NN, &ev);
    if (!f64) {
        PCR_REQUIRE(!t->is_voxel, "pcr_nn_query needs a point target (use pcr_nn_query_f64 for voxels)");
        const double b = r_max * (1.0 + 1e-6);
        launch_nn_query(t, 0, ctx->stream, d_q, m, bounded ? b * b : inf, rmax, d_dist, d_idx);
    } else if (!t->is_voxel) {
        PCR_REQUIRE(t->pts64 != nullptr, "pcr_nn_query_f64 needs a voxel target or a point target with float64 coordinates (pcr_target_points_set_f64)");
        // the float32 search must reach every point whose FLOAT64 position lies within r_max: r_max + band, a little more
        const double b = (r_max + t->band64) * 1.00002;
        launch_nn_query(t, 2, ctx->stream, d_q, m, bounded ? b * b * 1.000001 : inf, rmax, d_dist, d_idx);
    } else {
        const double b = r_max * (1.0 + 1e-6);
        launch_nn_query(t, 1, ctx->stream, d_q, m, bounded ? b * b : inf, rmax, d_dist, d_idx);
    }
    pcr_prof_end(ctx, &ev);
    HIP_TRY(hipGetLastError());
    return PCR_OK;
}
