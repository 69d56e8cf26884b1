// Single-process multi-device groups (round 6; VERDICT r5 item 3, SURVEY.md section 8b: "pcr_init(device_ids, n_dev) ... the
// scan sharded across devices inside pcr_scan_create").
//
// The reference is ONE process: a user calls set_target / align from one script (registration.py:28,71;
// demo_matching.py:147-152).  A group gives that script every GPU of the node without torchrun: one pcr_context + one host
// thread per member device, targets built once per member (the index is replicated), a scan cut into
// contiguous shards (the same bounds as distributed.shard_bounds), and per pass / per iteration ONE exchange of the 29 sums
// through the peer-to-peer transport of comm.hip -- here with plain in-process peer pointers (hipDeviceEnablePeerAccess; no IPC
// handles, no RCCL, no torch in the loop).  Every member runs the same device-resident Gauss-Newton loop on bit-identical
// sums, so a group call returns what the SPMD run with the same sharding returns, bit for bit.  device_ids may repeat:
// [0, 0] are two contexts (two streams) on one GPU, which is how the one-GPU test box exercises N > 1.
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <string.h>

#include "pcr_internal.h"

namespace {

// n persistent workers, member i on thread i: run(fn) executes fn(i) on every worker and returns when all are done
struct Workers {
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t gen = 0;
    int pending = 0;
    bool quit = false;
    const std::function<void(int)> *fn = nullptr;

    void start(int n) {
        for (int i = 0; i < n; ++i) threads.emplace_back([this, i] { loop(i); });
    }
    void loop(int i) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen;
                f = fn;
            }
            (*f)(i);
            {
                std::lock_guard<std::mutex> lk(mu);
                if (--pending == 0) cv_done.notify_all();
            }
        }
    }
    void run(const std::function<void(int)> &f) {
        std::unique_lock<std::mutex> lk(mu);
        fn = &f;
        pending = (int)threads.size();
        ++gen;
        cv_go.notify_all();
        cv_done.wait(lk, [&] { return pending == 0; });
        fn = nullptr;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv_go.notify_all();
        for (auto &t : threads) t.join();
        threads.clear();
    }
};

}   // namespace

struct pcr_group {
    std::vector<pcr_context *> ctx;
    Workers workers;
    int n() const { return (int)ctx.size(); }
};
struct pcr_group_target {
    pcr_group *g = nullptr;
    std::vector<pcr_target *> t;
};
struct pcr_group_scan {
    pcr_group *g = nullptr;
    std::vector<pcr_scan *> s;
    int64_t n = 0;
};

// fn(i) on every member's thread; the first failing member's status and message become the caller's
static pcr_status group_run(pcr_group *g, const std::function<pcr_status(int)> &fn) {
    const int n = g->n();
    std::vector<pcr_status> st((size_t)n, PCR_OK);
    std::vector<std::string> msg((size_t)n);
    if (n == 1) {                                   // no thread hop for the trivial group
        return fn(0);
    }
    const std::function<void(int)> body = [&](int i) {
        st[(size_t)i] = fn(i);
        if (st[(size_t)i] != PCR_OK) msg[(size_t)i] = pcr_last_error();
    };
    g->workers.run(body);
    for (int i = 0; i < n; ++i) {
        if (st[(size_t)i] != PCR_OK) {
            pcr_set_error("group member %d (device %d): %s", i, g->ctx[(size_t)i]->device, msg[(size_t)i].c_str());
            return st[(size_t)i];
        }
    }
    return PCR_OK;
}

extern "C" pcr_status pcr_group_create(const int *device_ids, int n, pcr_group **out) {
    PCR_REQUIRE(device_ids && out, "NULL argument");
    PCR_REQUIRE(n >= 1 && n <= 8, "a group has 1 to 8 members");
    pcr_group *g = new pcr_group();
    for (int i = 0; i < n; ++i) {
        pcr_context *c = nullptr;
        const pcr_status s = pcr_context_create(device_ids[i], &c);
        if (s != PCR_OK) {
            for (pcr_context *p : g->ctx) pcr_context_destroy(p);
            delete g;
            return s;
        }
        g->ctx.push_back(c);
    }
    const pcr_status s = pcr_comm_p2p_local(g->ctx.data(), n);
    if (s != PCR_OK) {
        for (pcr_context *p : g->ctx) pcr_context_destroy(p);
        delete g;
        return s;
    }
    if (n > 1) g->workers.start(n);
    *out = g;
    return PCR_OK;
}

extern "C" pcr_status pcr_group_destroy(pcr_group *g) {
    if (!g) return PCR_OK;
    g->workers.stop();
    for (pcr_context *p : g->ctx) pcr_context_destroy(p);
    delete g;
    return PCR_OK;
}

extern "C" pcr_status pcr_group_size(pcr_group *g, int *n) {
    PCR_REQUIRE(g && n, "NULL argument");
    *n = g->n();
    return PCR_OK;
}

// member i's context (borrowed: profiling, pipeline switches, pcr_context_synchronize); destroyed with the group
extern "C" pcr_status pcr_group_context(pcr_group *g, int i, pcr_context **ctx) {
    PCR_REQUIRE(g && ctx && i >= 0 && i < g->n(), "bad member index");
    *ctx = g->ctx[(size_t)i];
    return PCR_OK;
}

// ---- targets: the same index on every member ----------------------------------------------------------------------------
static void group_target_free(pcr_group_target *gt) {
    if (!gt) return;
    for (pcr_target *t : gt->t) pcr_target_destroy(t);
    delete gt;
}

extern "C" pcr_status pcr_group_target_points_create(pcr_group *g, const float *xyz, int64_t n, const float *normals_or_null,
                                                     float cell_hint, pcr_group_target **out) {
    PCR_REQUIRE(g && out && (xyz || n == 0), "NULL argument");
    pcr_group_target *gt = new pcr_group_target();
    gt->g = g;
    gt->t.assign((size_t)g->n(), nullptr);
    const pcr_status s = group_run(g, [&](int i) {
        return pcr_target_points_create(g->ctx[(size_t)i], xyz, n, normals_or_null, cell_hint, &gt->t[(size_t)i]);
    });
    if (s != PCR_OK) { group_target_free(gt); return s; }
    *out = gt;
    return PCR_OK;
}

extern "C" pcr_status pcr_group_target_voxels_create(pcr_group *g, const void *xyz, int xyz_is_f64, int64_t n, double voxel_size,
                                                     int min_points, pcr_group_target **out) {
    PCR_REQUIRE(g && out && (xyz || n == 0), "NULL argument");
    pcr_group_target *gt = new pcr_group_target();
    gt->g = g;
    gt->t.assign((size_t)g->n(), nullptr);
    const pcr_status s = group_run(g, [&](int i) {
        return pcr_target_voxels_create(g->ctx[(size_t)i], xyz, xyz_is_f64, n, voxel_size, min_points, &gt->t[(size_t)i]);
    });
    if (s != PCR_OK) { group_target_free(gt); return s; }
    *out = gt;
    return PCR_OK;
}

// normals_out (optional, [n][3]): member 0's -- every member computes the same ones
extern "C" pcr_status pcr_group_target_estimate_normals(pcr_group_target *gt, int k, int compat, float *normals_out) {
    PCR_REQUIRE(gt, "NULL argument");
    return group_run(gt->g, [&](int i) { return pcr_target_estimate_normals(gt->t[(size_t)i], k, compat, i == 0 ? normals_out : nullptr); });
}

extern "C" pcr_status pcr_group_target_set_normals(pcr_group_target *gt, const float *normals) {
    PCR_REQUIRE(gt && normals, "NULL argument");
    return group_run(gt->g, [&](int i) { return pcr_target_set_normals(gt->t[(size_t)i], normals); });
}

// quirk Q6 on every member (PCR_ERR_UNSUPPORTED, from all members alike, leaves the float32 search in place)
extern "C" pcr_status pcr_group_target_points_set_f64(pcr_group_target *gt, const double *xyz64) {
    PCR_REQUIRE(gt && xyz64, "NULL argument");
    return group_run(gt->g, [&](int i) { return pcr_target_points_set_f64(gt->t[(size_t)i], xyz64); });
}

// member i's target (borrowed: read-backs, pcr_nn_query, pcr_target_index_info ...)
extern "C" pcr_status pcr_group_target_member(pcr_group_target *gt, int i, pcr_target **t) {
    PCR_REQUIRE(gt && t && i >= 0 && i < (int)gt->t.size(), "bad member index");
    *t = gt->t[(size_t)i];
    return PCR_OK;
}

extern "C" pcr_status pcr_group_target_destroy(pcr_group_target *gt) {
    group_target_free(gt);
    return PCR_OK;
}

// ---- scans: contiguous shards, member i gets points [lo_i, hi_i) (distributed.shard_bounds) ------------------------------
static void shard_bounds(int64_t n, int rank, int world, int64_t *lo, int64_t *hi) {
    const int64_t base = n / world, rem = n % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
}

extern "C" pcr_status pcr_group_scan_create(pcr_group *g, const float *xyz, int64_t n, unsigned flags, pcr_group_scan **out) {
    PCR_REQUIRE(g && out && (xyz || n == 0), "NULL argument");
    pcr_group_scan *gs = new pcr_group_scan();
    gs->g = g; gs->n = n;
    gs->s.assign((size_t)g->n(), nullptr);
    const pcr_status s = group_run(g, [&](int i) {
        int64_t lo, hi;
        shard_bounds(n, i, g->n(), &lo, &hi);
        return pcr_scan_create(g->ctx[(size_t)i], xyz ? xyz + 3 * lo : nullptr, hi - lo, flags, &gs->s[(size_t)i]);
    });
    if (s != PCR_OK) {
        for (pcr_scan *p : gs->s) pcr_scan_destroy(p);
        delete gs;
        return s;
    }
    *out = gs;
    return PCR_OK;
}

extern "C" pcr_status pcr_group_scan_size(pcr_group_scan *gs, int64_t *n) {
    PCR_REQUIRE(gs && n, "NULL argument");
    *n = gs->n;
    return PCR_OK;
}

// member i's shard (borrowed: pcr_scan_read_matches, pcr_scan_reuse_stats ...); destroyed with the group scan
extern "C" pcr_status pcr_group_scan_member(pcr_group_scan *gs, int i, pcr_scan **s) {
    PCR_REQUIRE(gs && s && i >= 0 && i < (int)gs->s.size(), "bad member index");
    *s = gs->s[(size_t)i];
    return PCR_OK;
}

extern "C" pcr_status pcr_group_scan_destroy(pcr_group_scan *gs) {
    if (!gs) return PCR_OK;
    for (pcr_scan *p : gs->s) pcr_scan_destroy(p);
    delete gs;
    return PCR_OK;
}

// ---- the hot path over a group: calc_H_g_e2 / align of the WHOLE scan ---------------------------------------------------
extern "C" pcr_status pcr_group_linearize(pcr_group_target *gt, pcr_group_scan *gs, int kind, const double T[16], double max_dist,
                                          unsigned flags, double out[29]) {
    PCR_REQUIRE(gt && gs && T && out && gt->g == gs->g, "NULL argument, or target and scan of different groups");
    pcr_group *g = gt->g;
    flags &= ~(unsigned)PCR_FLAG_LOCAL_ONLY;                      // a group call is the sum over its members by definition
    std::vector<double> outs((size_t)g->n() * 29, 0.0);
    PCR_TRY(group_run(g, [&](int i) {
        return pcr_linearize(gt->t[(size_t)i], gs->s[(size_t)i], kind, T, max_dist, flags, outs.data() + (size_t)i * 29);
    }));
    // every member must hold the same, bit-identical sums: a member that read a stale slot or summed in another order would
    // take another Gauss-Newton step than member 0, whose copy is the one returned
    for (int i = 1; i < g->n(); ++i) {
        if (memcmp(outs.data() + (size_t)i * 29, outs.data(), 29 * sizeof(double)) != 0) {
            pcr_set_error("group member %d (device %d): its exchanged sums differ from member 0's", i, g->ctx[(size_t)i]->device);
            return PCR_ERR_COMM;
        }
    }
    memcpy(out, outs.data(), 29 * sizeof(double));
    return PCR_OK;
}

extern "C" pcr_status pcr_group_align(pcr_group_target *gt, pcr_group_scan *gs, int kind, const double T_init[16], int max_iter,
                                      double tol, double max_dist, unsigned flags, double T_out[16], int *iterations,
                                      double *trace_or_null) {
    PCR_REQUIRE(gt && gs && T_init && T_out && gt->g == gs->g, "NULL argument, or target and scan of different groups");
    pcr_group *g = gt->g;
    flags &= ~(unsigned)PCR_FLAG_LOCAL_ONLY;
    const int n = g->n();
    std::vector<double> Ts((size_t)n * 16, 0.0);
    std::vector<int> its((size_t)n, 0);
    std::vector<pcr_status> sts((size_t)n, PCR_OK);
    // with a trace wanted, every member writes its own (member 0's into the caller's buffer) so that the sums of every
    // iteration are compared, not only where they led
    const size_t trace_len = trace_or_null && max_iter > 0 ? (size_t)max_iter * 45 : 0;
    std::vector<double> traces(trace_len * (size_t)(n > 1 ? n - 1 : 0), 0.0);
    const pcr_status s = group_run(g, [&](int i) {
        double *tr = trace_len == 0 ? nullptr : i == 0 ? trace_or_null : traces.data() + (size_t)(i - 1) * trace_len;
        sts[(size_t)i] = pcr_align(gt->t[(size_t)i], gs->s[(size_t)i], kind, T_init, max_iter, tol, max_dist, flags,
                                   Ts.data() + (size_t)i * 16, &its[(size_t)i], tr);
        return sts[(size_t)i];
    });
    memcpy(T_out, Ts.data(), 16 * sizeof(double));
    if (iterations) *iterations = its[0];
    // every member must end alike: same status, iteration count, pose and (traced) per-iteration sums as member 0
    for (int i = 1; i < n; ++i) {
        const char *what = sts[(size_t)i] != sts[0] ? "status" : its[(size_t)i] != its[0] ? "iteration count"
                         : memcmp(Ts.data() + (size_t)i * 16, Ts.data(), 16 * sizeof(double)) != 0 ? "pose" : nullptr;
        if (!what && trace_len && its[0] > 0 &&
            memcmp(traces.data() + (size_t)(i - 1) * trace_len, trace_or_null, (size_t)its[0] * 45 * sizeof(double)) != 0)
            what = "trace";
        if (what) {
            pcr_set_error("group member %d (device %d): its %s differs from member 0's (status %d / %d, %d / %d iterations)", i,
                          g->ctx[(size_t)i]->device, what, sts[(size_t)i], sts[0], its[(size_t)i], its[0]);
            return PCR_ERR_COMM;
        }
    }
    return s;
}
