// K8  ilqr_solve -- the iLQR / DDP outer loop as ONE C-ABI call: the host side of the iteration (launch sequence, compacted
// list of still-active trajectories, termination test) runs here in C++ instead of in Python.
//
// Replaces: zopt/ilqrUtils.py:290-327 (iterativeLqr) and :360-397 (differentialDynamicProgramming), per trajectory
//     policy = (uGuess, 0); traj = rollout(x0, policy, zeros); J = cost(traj)                                   (:293-298)
//     while not converged and it < maxIter:                                                                      (:301-303)
//         expansions along traj; PD-conditioned Hessians; backward pass; 16-way line search; converged = |J - Jn| <= tol
// on a batch: every kernel runs over the compacted id list of the trajectories that have not converged yet (rebuilt on the
// device every `sync_every` iterations, when the host also learns how many are left), converged trajectories drop out.
// The kernels are the ones behind the array-level entry points (linearize.hip, ilqr_backward.hip, rollout*.hip, psd.hip);
// nothing is allocated here: the caller provides the workspace (zm_ilqr_solve_workspace_f64 tells how much).
#include <utility>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "input_box.h"
#include "models.h"
#include "quad_derivs_gen.h"
#include "state_box.h"
#include "track_cost.h"
#include "traced_con.h"
#include "traced_cost.h"
#include "zm_common.h"

namespace zm {

// Stable compaction of the active ids (ascending trajectory order, as torch.nonzero gave the Python loop): one block, one
// ballot-scan pass per 1024 trajectories.  count[0] <- number of active trajectories.
// hostword (pinned host memory, may be null): <- (seq << 32 | count) as ONE 8-byte system-scope store -- the host side of the solve
// polls it instead of waiting for a copy kernel, an event and the interrupt behind hipEventSynchronize (~45 us per round trip).
__global__ __launch_bounds__(1024) void compact_active_kernel(const int* __restrict__ active, const long batch, int* __restrict__ list,
                                                              int* __restrict__ count, unsigned long long* hostword,
                                                              const unsigned seq) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (long start = 0; start < batch; start += 1024) {
        const long i = start + tid;
        const bool a = i < batch && active[i] != 0;
        const unsigned long long m = __ballot(a);
        const int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __builtin_popcountll(m);
        __syncthreads();
        int off = base;
        for (int j = 0; j < w; ++j) off += wsum[j];
        if (a) list[off + before] = (int)i;
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int j = 0; j < 16; ++j) s += wsum[j];
            base += s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        count[0] = base;
        if (hostword) __hip_atomic_store(hostword, ((unsigned long long)seq << 32) | (unsigned)base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Start of a solve in ONE launch (it was seven memset / memcpy / fill calls, each a runtime call of its own on the host):
// l <- uGuess, L <- 0 (policy0 = (uGuess, 0), ilqrUtils.py:293), previous trajectory <- 0 (:294), alphas <- 0.5 ** arange(16) (:145),
// active <- 1, converged <- 0, where <- 0.
__global__ __launch_bounds__(256) void ilqr_init_kernel(double* __restrict__ l, const double* __restrict__ uGuess, const long nl,
                                                        double* __restrict__ L, const long nL, double* __restrict__ xT2, const long nx,
                                                        double* __restrict__ uT2, double* __restrict__ alphas, int* __restrict__ active,
                                                        int* __restrict__ converged, int* __restrict__ where, const long batch) {
    const long stride = (long)gridDim.x * blockDim.x, t0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long i = t0; i < nL; i += stride) L[i] = 0.0;
    for (long i = t0; i < nx; i += stride) xT2[i] = 0.0;
    for (long i = t0; i < nl; i += stride) {
        l[i] = uGuess[i];
        uT2[i] = 0.0;
    }
    for (long i = t0; i < batch; i += stride) {
        active[i] = 1;
        converged[i] = 0;
        if (where) where[i] = 0;
    }
    if (t0 < 16) alphas[t0] = 1.0 / (double)(1u << t0);   // exact powers of two
}

__global__ void fill_i32_kernel(int* __restrict__ p, const long n, const int v) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ void fill_alphas_kernel(double* __restrict__ a) {
    a[threadIdx.x] = 1.0 / (double)(1u << threadIdx.x);   // exact powers of two
}

__global__ void fill_f64_kernel(double* __restrict__ p, const long n, const double v) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

struct IlqrWs {   // carve of the caller's workspace (doubles)
    long l, xT2, uT2, Jn, f_x, f_u, c_x, c_u, v_x, c_xx, c_ux, c_uu, v_xx, alphas, f_xx, f_ux, f_uu, idx, where, scratch, tail_slots, total;
};

// Once at most this many trajectories are left, the line search runs in all-store mode (rollout_fast.hip): its 16 rollouts per
// trajectory go to scratch rows and the accept step copies the winner, instead of re-rolling the winner in a second pass of T more
// dependent steps.  With few trajectories a launch lasts as long as one wave's chain, so this halves it; with many, the 16x stores
// (207 KB per trajectory at n=12, m=4, T=100) would cost more HBM time than the second pass costs ALU time.
// ZOPT_AMD_ILQR_TAIL=<n> overrides the threshold (0: never).
constexpr long ILQR_TAIL_DEFAULT = 2048;
static long ilqr_tail_slots(long batch) {
    static const long thr = [] {
        const char* e = zm::lab_env("ZOPT_AMD_ILQR_TAIL");
        return e ? atol(e) : ILQR_TAIL_DEFAULT;
    }();
    return thr < 0 ? 0 : (thr < batch ? thr : batch);
}

int expand_list(const zm_model_t* model, const zm_quadcost_t* cost, const double* xTraj, const double* uTraj, const int32_t* list,
                int64_t count, const int32_t* active, double* f_x, double* f_u, double* c_x, double* c_u, double* v_x, int64_t batch,
                int T, void* stream, int packed, const TrackRef* track);
struct TrajList {
    const int* list;
    long count;
};
int sweep_packed_jacobians(const double* Fp, int njp, const unsigned char* pos, const double* Hpk, const PairTab& ptab, const double* c_x,
                           const double* c_u, const double* c_xx, const double* c_ux, const double* c_uu, const double* vf_x,
                           const double* vf_xx, const int* act, double* l, double* L, int64_t batch, int T, hipStream_t st, TrajList tl,
                           int nhs, const unsigned short* hdense, int nh);
int quad_hessian_sparse_list(const zm_model_t* model, const double* xTraj, const double* uTraj, const int32_t* list, int64_t count,
                             const int32_t* active, double* Hs, int64_t batch, int T, void* stream);
bool rollout_all_store_supported(const zm_model_t* model, const zm_quadcost_t* cost, int T);
bool rollout_all_store_model_ok(const zm_model_t* model);
int rollout_linesearch_all_store(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* l, const double* L,
                                 const double* xPrev, const double* uPrev, const double* alphas, const int32_t* list, int64_t count,
                                 const int32_t* active, double* scratch, double* J, int32_t* alpha_idx, int64_t batch, int T,
                                 void* stream, const TrackRef* track);
int ilqr_accept(const int32_t* list, int64_t count, double* J, const double* Jn, double* xTraj, const double* xTrajNew, double* uTraj,
                const double* uTrajNew, int32_t* converged, int32_t* active, double tol, int64_t batch, int T, int n, int m,
                void* stream, const double* scratch, const int32_t* idx, int32_t* where, int where_val);
int ilqr_collect(const int32_t* where, double* xTraj, const double* xAlt, double* uTraj, const double* uAlt, int64_t batch, int T, int n,
                 int m, void* stream);

// state_box.hip
int ilqr_init_masked(const int32_t* mask, double* l, const double* uStart, double* L, double* xT2, double* uT2, double* alphas,
                     int32_t* active, int32_t* converged, int32_t* where, int64_t batch, int T, int n, int m, hipStream_t st);
int state_penalty_expand(const zm_statebox_t* sbox, const double* xTraj, const int32_t* list, int64_t count, const int32_t* active,
                         double* c_x, double* v_x, double* h, int32_t* visits, int64_t batch, int T, int n, hipStream_t st);

// One inner solve of the augmented-Lagrangian loop (zm_ilqr_solve_state_f64): the loop below on J_AL = cost + penalty of the state box.
struct StatePen {
    const zm_statebox_t* sbox;
    double* h;                  // (batch, T+1, n) diagonal addend of the cost Hessians, written by the penalty expansion
    double* Jcost;              // (batch) the cost without the penalty, written by the line search's store pass
    int32_t* visits;            // (batch, optional) += 1 per iteration of the loop over the trajectory
    const int32_t* init_mask;   // (batch) the trajectories this inner solve covers; the others are skipped by the init kernel, the
                                // initial rollout and the loop
    const double* uStart;       // (batch, T, m) the inputs it starts from
};

// The cost of a solve, as the loop sees it: the resolved cost (track_cost.h: one loop serves zm_quadcost_t and zm_trackcost_t) and
// what the box and state entries add to it.
struct IlqrCost : CostRef {
    // input bounds (zm_ilqr_solve_box_f64; nullptr: none): the sweep (iLQR or DDP) and the line search are then the box forms
    const zm_inputbox_t* box = nullptr;
    int32_t* qp_capped = nullptr;
    // state box (zm_ilqr_solve_state_f64; nullptr: none): penalty line search, penalty expansion, sweep with the diagonal addend
    const StatePen* pen = nullptr;
    // recorded cost (zm_traced_cost_solve_f64; nullptr: none): its own line search and expansion, per-point Hessians conditioned in
    // every iteration, the list sweeps with shared_hessian = 0; there are then no weights, no box and no penalty
    const zm_tracedcost_t* traced = nullptr;
    // recorded constraints (zm_traced_con_solve_f64; nullptr: none): their own penalty line search, the cost's expansion followed by the
    // penalty's into per-point Hessians (shared conditioned set + Gauss-Newton addend), the list sweeps with shared_hessian = 0
    const struct ConPen* con = nullptr;
};
// One inner solve of the augmented-Lagrangian loop on recorded constraints (zm_traced_con_solve_f64): StatePen's part there.
struct ConPen {
    const zm_tracedcon_t* tc;
    double *sc_xx, *sc_ux, *sc_uu, *sv_xx;   // the shared Hessians of the quadratic cost, PD-conditioned once per inner solve
    double* Jcost;              // (batch) the cost without the penalty, written by the line search's store pass
    int32_t* visits;            // (batch, optional) += 1 per iteration of the loop over the trajectory
    const int32_t* init_mask;   // (batch) the trajectories this inner solve covers
    const double* uStart;       // (batch, T, m) the inputs it starts from
};
// psd.hip: the projections of zm_condition_cost_f64 / zm_psd_project_f64 over the listed trajectories' per-point Hessians
int condition_cost_listed(double* c_xx, double* c_ux, double* c_uu, const int* list, long count, int T, int n, int m, double eps,
                          hipStream_t st);
int psd_project_listed(double* A, const int* list, long count, int k, double eps, hipStream_t st);
// the line search of the loop: dense (list == nullptr) or over the id list
static int cost_linesearch(const IlqrCost& ck, const zm_model_t* model, const double* x0, const double* l, const double* L,
                           const double* xPrev, const double* uPrev, const double* alphas, int n_alpha, const int32_t* list,
                           int64_t count, const int32_t* active, double* xTraj, double* uTraj, double* J, int32_t* alpha_idx,
                           int64_t batch, int T, void* stream) {
    if (ck.traced)
        return zm_traced_cost_linesearch_list_f64(model, ck.traced, x0, l, L, xPrev, uPrev, alphas, n_alpha, list, count, active, xTraj,
                                                  uTraj, J, alpha_idx, batch, T, stream);
    if (ck.con)
        return zm_traced_con_linesearch_list_f64(model, ck.track ? nullptr : &ck.w, ck.track, ck.con->tc, x0, l, L, xPrev, uPrev, alphas,
                                                 n_alpha, list, count, active, xTraj, uTraj, J, ck.con->Jcost, alpha_idx, batch, T,
                                                 stream);
    if (ck.pen)
        return zm_rollout_linesearch_state_list_f64(model, ck.track ? nullptr : &ck.w, ck.track, ck.box, ck.pen->sbox, x0, l, L, xPrev,
                                                    uPrev, alphas, n_alpha, list, count, active, xTraj, uTraj, J, ck.pen->Jcost,
                                                    alpha_idx, batch, T, stream);
    if (ck.box)
        return zm_rollout_linesearch_box_list_f64(model, ck.track ? nullptr : &ck.w, ck.track, ck.box, x0, l, L, xPrev, uPrev, alphas,
                                                  n_alpha, list, count, active, xTraj, uTraj, J, alpha_idx, batch, T, stream);
    if (ck.track)
        return zm_rollout_linesearch_tracking_list_f64(model, ck.track, x0, l, L, xPrev, uPrev, alphas, n_alpha, list, count, active, xTraj,
                                                       uTraj, J, alpha_idx, batch, T, stream);
    if (list)
        return zm_rollout_linesearch_list_f64(model, &ck.w, x0, l, L, xPrev, uPrev, alphas, n_alpha, list, count, active, xTraj, uTraj, J,
                                              alpha_idx, batch, T, stream);
    return zm_rollout_linesearch_f64(model, &ck.w, x0, l, L, xPrev, uPrev, alphas, n_alpha, active, xTraj, uTraj, J, alpha_idx, batch, T,
                                     stream);
}

// per_point: the cost Hessians are (batch, T, ...) / (batch, n, n) arrays (a recorded cost) instead of one shared set, and there is no
// all-store block: the workspace grows by batch*T*(n*n + m*n + m*m) + batch*n*n doubles less the shared set
static IlqrWs carve(const zm_model_t* model, long b, long T, int ddp, int need_ux, int npairs, bool per_point = false) {
    const long n = model->n, m = model->m;
    IlqrWs w;
    long o = 0;
    auto take = [&](long cnt) {
        const long at = o;
        o += (cnt + 1) & ~1L;   // 16-B aligned pieces (the sweep kernels' DMA path needs it)
        return at;
    };
    w.l = take(b * T * m);
    w.xT2 = take(b * (T + 1) * n);
    w.uT2 = take(b * T * m);
    w.Jn = take(b);
    w.f_x = take(b * T * n * n);
    w.f_u = take(b * T * n * m);
    w.c_x = take(b * T * n);
    w.c_u = take(b * T * m);
    w.v_x = take(b * n);
    w.c_xx = take(per_point ? b * T * n * n : n * n);
    w.c_ux = take(per_point ? b * T * m * n : m * n);
    w.c_uu = take(per_point ? b * T * m * m : m * m);
    w.v_xx = take(per_point ? b * n * n : n * n);
    w.alphas = take(16);
    // second derivatives: packed (pairs x n per point) when the model declares its nonzero pairs, else the full tensors
    w.f_xx = ddp ? take(npairs > 0 ? b * T * npairs * n : b * T * n * n * n) : 0;
    w.f_ux = (ddp && need_ux && npairs == 0) ? take(b * T * n * m * n) : 0;
    w.f_uu = (ddp && need_ux && npairs == 0) ? take(b * T * n * m * m) : 0;
    w.idx = take((b + 1) / 2);   // int32 winner index per trajectory
    w.where = take((b + 1) / 2); // int32 per trajectory: 0 = newest rows in the caller's xTraj / uTraj, 1 = in xT2 / uT2
    // all-store blocks (16 step sizes x 16 doubles per step and slot: 423 MB at T = 100 for 2048 slots) only for the models whose line
    // search can run in that form -- a windy quadcopter, another model or the generic rollout path never touch them
    w.tail_slots = (!per_point && rollout_all_store_model_ok(model)) ? ilqr_tail_slots(b) : 0;
    w.scratch = take(w.tail_slots * (T + 1) * 256);
    w.total = o;
    return w;
}

// What the backward sweep of a solve runs on, decided once before the loop: the form of the Jacobians and of the second derivatives.
struct SweepPlan {
    int ddp, npairs;
    bool packed, sparse_h;
    double *f_ux, *f_uu;   // nullptr: identically zero (a model affine in its controls) or held as pairs -- neither written nor read
    int njp;
    const unsigned char* jpos;
    PairTab ptab;
    int nh, nhs;
    const unsigned short* hdense;
};
static SweepPlan sweep_plan(const zm_model_t* model, const IlqrCost& ck, double* ws, const IlqrWs& w, int ddp, int need_ux, int npairs) {
    // Packed Jacobians (quadcopter): the expansion writes and the ring sweeps read only the structurally nonzero entries of
    // [f_x | f_u] -- 448 B (480 with wind) per point instead of 1 536 B.  ZOPT_AMD_JAC=full or ZOPT_AMD_ILQR_PATH=reg: the full matrices.
    // (a box solve: full Jacobians only)
    static const bool packed_off = [] {
        const char* e = zm::lab_env("ZOPT_AMD_JAC");
        const char* r = zm::fallback_env("ZOPT_AMD_ILQR_PATH");
        return (e && e[0] == 'f') || (r && r[0] == 'r');
    }();
    // ... and the DDP path's second derivatives SPARSE (69 / 85 structurally nonzero entries of the 28 x 12 per point; ZOPT_AMD_HES=dense:
    // the dense pair rows)
    static const bool sparse_off = [] {
        const char* e = zm::lab_env("ZOPT_AMD_HES");
        return e && e[0] == 'd';
    }();
    const bool windy = model->wind_ned[0] != 0.0 || model->wind_ned[1] != 0.0 || model->wind_ned[2] != 0.0;
    SweepPlan p;
    p.ddp = ddp, p.npairs = npairs;
    p.packed = !ck.box && !ck.pen && !ck.traced && !ck.con && !packed_off && model->kind == ZM_MODEL_QUADCOPTER && model->dt != 0.0 &&
               (((uintptr_t)ws) & 15) == 0 && (!ddp || npairs == 28);
    p.sparse_h = p.packed && ddp && !sparse_off;
    p.f_ux = (need_ux && npairs == 0) ? ws + w.f_ux : nullptr;
    p.f_uu = (need_ux && npairs == 0) ? ws + w.f_uu : nullptr;
    p.njp = windy ? ((QUAD_NJ_WIND + 1) & ~1) : ((QUAD_NJ_STILL + 1) & ~1);
    p.jpos = windy ? QUAD_JPOS_WIND : QUAD_JPOS_STILL;
    p.ptab = model_pair_table(model->kind);
    p.nh = windy ? QUAD_NH_WIND : QUAD_NH_STILL, p.nhs = (p.nh + 1) & ~1;
    p.hdense = windy ? QUAD_HDENSE_WIND : QUAD_HDENSE_STILL;
    return p;
}

// The backward pass of one iteration over the listed trajectories (for DDP behind its second derivatives along curX, curU): the form
// that the plan and the cost's box / penalty select.  l goes to the workspace, L to the caller's array.
static int backward_sweep(const SweepPlan& p, const IlqrCost& ck, const zm_model_t* model, double* ws, const IlqrWs& w, const double* curX,
                          const double* curU, const int32_t* list, int64_t count, const int32_t* active, double* L, int64_t batch, int T,
                          hipStream_t st) {
    const int n = model->n, m = model->m;
    const int shared = (ck.traced || ck.con) ? 0 : 1;   // shared_hessian of the plain sweeps: a recorded cost or constraint has per-point Hessians
    int rc = ZM_OK;
    if (p.packed) {
        if (p.sparse_h)
            rc = quad_hessian_sparse_list(model, curX, curU, list, count, active, ws + w.f_xx, batch, T, st);
        else if (p.ddp)
            rc = zm_quadratic_dynamics_pairs_list_f64(model, curX, curU, list, count, active, ws + w.f_xx, batch, T, st);
        if (rc) return rc;
        rc = sweep_packed_jacobians(ws + w.f_x, p.njp, p.jpos, p.ddp ? ws + w.f_xx : nullptr, p.ptab, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                    ws + w.c_ux, ws + w.c_uu, ws + w.v_x, ws + w.v_xx, (const int*)active, ws + w.l, L, batch, T, st,
                                    TrajList{(const int*)list, (long)count}, p.sparse_h ? p.nhs : 0, p.hdense, p.nh);
        if (rc == ZM_EUNSUPPORTED) return set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_f64: packed sweep refused its operands");
        return rc;
    }
    if (p.ddp) {
        // The second derivatives as pairs where the model declares them -- 28 x 12 doubles per point for the quadcopter instead of the
        // zero-filled (n,n,n) tensors (2.7 KB instead of 13.8 KB written by the expansion and read back by the sweep, same arithmetic)
        // -- and as the full tensors otherwise.  With input bounds: the register sweep with the box-QP per step on the current inputs.
        if (p.npairs > 0) {
            rc = zm_quadratic_dynamics_pairs_list_f64(model, curX, curU, list, count, active, ws + w.f_xx, batch, T, st);
            if (rc) return rc;
            if (ck.box)
                return zm_ddp_backward_pairs_box_list_f64(model, ws + w.f_x, ws + w.f_u, ws + w.f_xx, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                                          ws + w.c_ux, ws + w.c_uu, ws + w.v_x, ws + w.v_xx, curU, ck.box, list, count,
                                                          active, 1, ws + w.l, L, ck.qp_capped, batch, T, st);
            return zm_ddp_backward_pairs_list_f64(model, ws + w.f_x, ws + w.f_u, ws + w.f_xx, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                                  ws + w.c_ux, ws + w.c_uu, ws + w.v_x, ws + w.v_xx, list, count, active, shared,
                                                  ws + w.l, L, batch, T, st);
        }
        rc = zm_quadratic_dynamics_list_f64(model, curX, curU, list, count, active, ws + w.f_xx, p.f_ux, p.f_uu, batch, T, st);
        if (rc) return rc;
        if (ck.box)
            return zm_ddp_backward_box_list_f64(ws + w.f_x, ws + w.f_u, ws + w.f_xx, p.f_ux, p.f_uu, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                                ws + w.c_ux, ws + w.c_uu, ws + w.v_x, ws + w.v_xx, curU, ck.box, list, count, active, 1,
                                                ws + w.l, L, ck.qp_capped, batch, T, n, m, st);
        return zm_ddp_backward_list_f64(ws + w.f_x, ws + w.f_u, ws + w.f_xx, p.f_ux, p.f_uu, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                        ws + w.c_ux, ws + w.c_uu, ws + w.v_x, ws + w.v_xx, list, count, active, shared, ws + w.l, L,
                                        batch, T, n, m, st);
    }
    if (ck.pen)
        return zm_ilqr_backward_state_list_f64(ws + w.f_x, ws + w.f_u, ws + w.c_x, ws + w.c_u, ws + w.c_xx, ws + w.c_ux, ws + w.c_uu,
                                               ws + w.v_x, ws + w.v_xx, ck.pen->h, ck.box ? curU : nullptr, ck.box, list, count, active,
                                               1, ws + w.l, L, ck.qp_capped, batch, T, n, m, st);
    if (ck.box)
        return zm_ilqr_backward_box_list_f64(ws + w.f_x, ws + w.f_u, ws + w.c_x, ws + w.c_u, ws + w.c_xx, ws + w.c_ux, ws + w.c_uu,
                                             ws + w.v_x, ws + w.v_xx, curU, ck.box, list, count, active, 1, ws + w.l, L, ck.qp_capped,
                                             batch, T, n, m, st);
    return zm_ilqr_backward_list_f64(ws + w.f_x, ws + w.f_u, ws + w.c_x, ws + w.c_u, ws + w.c_xx, ws + w.c_ux, ws + w.c_uu, ws + w.v_x,
                                     ws + w.v_xx, list, count, active, shared, ws + w.l, L, batch, T, n, m, st);
}

// Pool of (pinned int32, event) pairs per device for the drivers' host round trips.
struct HostSlot {
    int dev;
    unsigned long long* word;   // pinned: (seq << 32 | count), written by compact_active_kernel
    hipEvent_t event;
    bool busy;
    unsigned seq;               // last sequence number handed out for this word
};
static std::mutex g_slot_mutex;
static std::vector<HostSlot> g_slots;

class HostSlotLease {
  public:
    explicit HostSlotLease(int dev) : idx_(-1) {
        std::lock_guard<std::mutex> lk(g_slot_mutex);
        for (size_t i = 0; i < g_slots.size(); ++i)
            if (g_slots[i].dev == dev && !g_slots[i].busy) {
                g_slots[i].busy = true;
                idx_ = (long)i;
                word_ = g_slots[i].word;
                event_ = g_slots[i].event;
                return;
            }
        HostSlot s{dev, nullptr, nullptr, true, 0u};
        if (hipHostMalloc((void**)&s.word, sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) return;
        *s.word = 0ull;
        if (hipEventCreateWithFlags(&s.event, hipEventDisableTiming) != hipSuccess) {
            (void)hipHostFree(s.word);
            return;
        }
        g_slots.push_back(s);
        idx_ = (long)g_slots.size() - 1;
        word_ = s.word;
        event_ = s.event;
    }
    ~HostSlotLease() {
        if (idx_ < 0) return;
        std::lock_guard<std::mutex> lk(g_slot_mutex);
        if ((size_t)idx_ < g_slots.size() && g_slots[idx_].word == word_) g_slots[idx_].busy = false;
    }
    bool ok() const { return idx_ >= 0; }
    unsigned long long* word() const { return word_; }
    hipEvent_t event() const { return event_; }
    unsigned next_seq() {   // a fresh tag per round trip (never 0: the word starts as 0)
        std::lock_guard<std::mutex> lk(g_slot_mutex);
        unsigned& q = g_slots[idx_].seq;
        q = (q == 0xffffffffu) ? 1u : q + 1u;
        return q;
    }

  private:
    long idx_;
    unsigned long long* word_ = nullptr;
    hipEvent_t event_ = nullptr;
};

// Waits until the device has published (seq, count) in the pinned word; returns count.  Busy-polls (the answer is a few
// microseconds away: one small kernel behind what is already queued); after `spin_limit` polls without it -- a slow or
// profiled run -- it falls back to the event behind the kernel and the device-side copy of the count.
static int wait_for_count(const unsigned long long* word, const unsigned seq, hipEvent_t ev, const int32_t* dcount, int32_t* out) {
    for (long spin = 0; spin < 20000000L; ++spin) {
        const unsigned long long v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        if ((unsigned)(v >> 32) == seq) {
            *out = (int32_t)(unsigned)(v & 0xffffffffull);
            return ZM_OK;
        }
        __builtin_ia32_pause();
    }
    ZM_HIP_CHECK(hipEventSynchronize(ev));
    ZM_HIP_CHECK(hipMemcpy(out, dcount, sizeof(int32_t), hipMemcpyDeviceToHost));
    return ZM_OK;
}

// zm_shutdown(): frees every pair that is not lent out; returns how many were released.
int release_host_slots() {
    std::lock_guard<std::mutex> lk(g_slot_mutex);
    int freed = 0;
    std::vector<HostSlot> keep;
    for (auto& s : g_slots) {
        if (s.busy) {
            keep.push_back(s);
            continue;
        }
        (void)hipEventDestroy(s.event);
        (void)hipHostFree(s.word);
        ++freed;
    }
    g_slots.swap(keep);
    return freed;
}

}  // namespace zm

extern "C" int64_t zm_ilqr_solve_workspace_f64(const zm_model_t* model, int64_t batch, int T, int ddp) {
    if (!model || batch < 0 || T < 1) return -1;
    uint32_t mask = 0;
    int32_t npairs = 0;
    if (ddp && (zm_model_nonlinear_mask(model, &mask) != ZM_OK || zm_model_hessian_pairs(model, nullptr, &npairs) != ZM_OK)) return -1;
    return zm::carve(model, batch, T, ddp, (mask >> model->n) != 0, npairs).total;
}

// One fused solve as its entry received it: every zm_ilqr_solve*_f64 entry fills this record and hands it to ilqr_solve_impl.
struct SolveCall {
    const zm_model_t* model;
    zm::IlqrCost ck;
    const double *x0, *uGuess;
    int ddp, max_iter;
    double tol;
    int sync_every;
    double* workspace;
    int64_t workspace_doubles;
    int32_t* iwork;
    double *xTraj, *uTraj, *L, *J;
    int32_t *converged, *iterations;
    int64_t batch;
    int T;
    void* stream;
    double* J_trace = nullptr;
    int32_t* alpha_trace = nullptr;
};

static int ilqr_solve_impl(const SolveCall& c) {
    const zm_model_t* const model = c.model;
    const zm::IlqrCost& ck = c.ck;
    const int64_t batch = c.batch;
    const int T = c.T, ddp = c.ddp;
    double *const xTraj = c.xTraj, *const uTraj = c.uTraj, *const L = c.L, *const J = c.J;
    if (batch == 0) return ZM_OK;
    const zm_quadcost_t* cost = ck.weights();
    if (!model || (!cost && !ck.traced) || !c.x0 || !c.uGuess || !c.workspace || !c.iwork || !xTraj || !uTraj || !L || !J || !c.converged)
        return zm::set_error(ZM_EINVAL, "zm_ilqr_solve_f64: null pointer");
    if (batch < 0 || T < 1 || c.max_iter < 0 || c.sync_every < 1) return zm::set_error(ZM_EINVAL, "zm_ilqr_solve_f64: bad size");
    const int n = model->n, m = model->m;
    if (ck.traced && (cost || ck.track || ck.box || ck.pen || n != ck.traced->n || m != ck.traced->m))
        return zm::set_error(ZM_EUNSUPPORTED, "zm_traced_cost_solve_f64: a recorded cost of the model's (n, m) and nothing else (weights, "
                                              "input box and state box next to a recorded cost are not built)");
    if (ck.con && (ddp || cost == nullptr || ck.box || ck.pen || ck.traced || n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM))
        return zm::set_error(ZM_EUNSUPPORTED, "zm_traced_con_solve_f64: iLQR on a quadratic or tracking cost with n<=12, m<=4 and nothing "
                                              "else (DDP, input box, state box and a recorded cost next to a recorded constraint are not "
                                              "built)");
    if (model->kind == ZM_MODEL_TRACED && (ck.track || ck.box || ck.pen))
        return zm::set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_f64: a traced model takes a zm_quadcost_t and no bounds (tracking cost, input "
                                              "box and state box on the tape interpreter are not built)");
    if (ck.box) {
        if (n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM)
            return zm::set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_box_f64: (n=%d, m=%d) not covered (input box: n<=12, m<=4)", n, m);
        if (const int rb = zm::box_check(ck.box, m, T, "zm_ilqr_solve_box_f64")) return rb;
        if (ck.qp_capped && !ck.pen) ZM_HIP_CHECK(hipMemsetAsync(ck.qp_capped, 0, sizeof(int32_t) * batch, (hipStream_t)c.stream));
    }
    if (ck.pen && (ddp || n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM))
        return zm::set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_state_f64: iLQR with n<=12, m<=4 only (n=%d, m=%d, ddp=%d)", n, m, ddp);
    if (ck.track && model->kind == ZM_MODEL_LINEAR && (n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM))
        return zm::set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_tracking_f64: (n=%d, m=%d) not covered (tracking cost: n<=12, m<=4)", n, m);
    uint32_t mask = 0;
    int32_t npairs = 0;
    if (ddp) {
        int rc = zm_model_nonlinear_mask(model, &mask);
        if (rc) return rc;
        rc = zm_model_hessian_pairs(model, nullptr, &npairs);
        if (rc) return rc;
    }
    const int need_ux = (mask >> n) != 0;   // a model affine in its controls has f_ux = f_uu = 0: neither written nor read
    const zm::IlqrWs w = zm::carve(model, batch, T, ddp, need_ux, npairs, ck.traced != nullptr || ck.con != nullptr);
    if (c.workspace_doubles < w.total)
        return zm::set_error(ZM_EINVAL, "zm_ilqr_solve_f64: workspace of %lld doubles, %lld needed", (long long)c.workspace_doubles,
                             (long long)w.total);
    hipStream_t st = (hipStream_t)c.stream;
    double* ws = c.workspace;
    // iwork (int32): active (batch) | list (batch) | count (2)
    int32_t* active = c.iwork;
    int32_t* list = c.iwork + batch;
    int32_t* dcount = c.iwork + 2 * batch;
    const long xrow = (long)(T + 1) * n, urow = (long)T * m;

    // policy = (uGuess, 0); traj_prev = zeros; step sizes; masks                                     (ilqrUtils.py:293-294, :145)
    int32_t* where = (int32_t*)(ws + w.where);
    const bool al = ck.pen || ck.con;   // an inner solve of an augmented-Lagrangian loop: masked start
    if (al) {
        const int ri = zm::ilqr_init_masked(ck.pen ? ck.pen->init_mask : ck.con->init_mask, ws + w.l,
                                            ck.pen ? ck.pen->uStart : ck.con->uStart, L, ws + w.xT2, ws + w.uT2, ws + w.alphas, active,
                                            c.converged, where, batch, T, n, m, st);
        if (ri) return ri;
    } else {
        const long nL = (long)batch * urow * n, nx = (long)batch * xrow, nl = (long)batch * urow;
        const long work = nL > nx ? nL : nx;
        const unsigned blocks = (unsigned)((work + 256L * 8 - 1) / (256L * 8) < 4096 ? (work + 256L * 8 - 1) / (256L * 8) : 4096);
        hipLaunchKernelGGL(zm::ilqr_init_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, ws + w.l, c.uGuess, nl, L, nL, ws + w.xT2, nx,
                           ws + w.uT2, ws + w.alphas, (int*)active, (int*)c.converged, (int*)where, (long)batch);
    }
    // initial rollout (alpha = 1) from the zero trajectory and its cost                                (:297-298)
    int rc = zm::cost_linesearch(ck, model, c.x0, ws + w.l, L, ws + w.xT2, ws + w.uT2, ws + w.alphas, 1, nullptr, 0,
                                 al ? active : nullptr, xTraj, uTraj, J, nullptr, batch, T, st);
    if (rc) return rc;
    // trajectory-independent Hessians of the quadratic cost, PD-conditioned once                         (:309-313)
    // (a recorded cost: per-point Hessians, expanded and conditioned in every iteration below)
    // (recorded constraints: the same shared set, kept beside the per-point arrays that the penalty expansion fills from it)
    if (!ck.traced) {
        double *const s_xx = ck.con ? ck.con->sc_xx : ws + w.c_xx, *const s_ux = ck.con ? ck.con->sc_ux : ws + w.c_ux,
                     *const s_uu = ck.con ? ck.con->sc_uu : ws + w.c_uu, *const s_vxx = ck.con ? ck.con->sv_xx : ws + w.v_xx;
        rc = zm_quadratize_cost_f64(cost, n, m, xTraj, uTraj, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s_xx, s_ux, s_uu,
                                    s_vxx, 0, T, st);
        if (rc) return rc;
        rc = zm_condition_cost_f64(s_xx, s_ux, s_uu, 1, n, m, 1e-3, st);
        if (rc) return rc;
        rc = zm_psd_project_f64(s_vxx, 1, n, 1e-3, st);
        if (rc) return rc;
    }

    // (a box solve: one-lane two-pass line search and full Jacobians only)
    const bool can_all_store = !ck.box && !ck.pen && w.tail_slots > 0 && zm::rollout_all_store_supported(model, cost, T);
    const zm::SweepPlan plan = zm::sweep_plan(model, ck, ws, w, ddp, need_ux, npairs);
    int32_t* widx = (int32_t*)(ws + w.idx);
    // pinned word + event for the active count, borrowed from a per-device pool for the duration of this call (a pinned allocation
    // per solve costs ~1 ms; an event belongs to the device that was current when it was created).  Concurrent solves on one device
    // get distinct pairs; zm_shutdown() releases the pool.
    int dev = 0;
    ZM_HIP_CHECK(hipGetDevice(&dev));
    zm::HostSlotLease lease(dev);
    if (!lease.ok()) return zm::set_error(ZM_EUNSUPPORTED, "zm_ilqr_solve_f64: cannot get a pinned word / event on device %d", dev);
    unsigned long long* const hword = lease.word();
    const hipEvent_t count_ready = lease.event();
    // The trajectories alternate between two buffers: the two-pass line search reads the current rows (xPrev, uPrev) and writes the
    // winner's into the other buffer, which then IS the current one -- the acceptance step copies nothing (it was 212 MB per
    // full-batch iteration).  Every active trajectory is rewritten in every iteration, so the current buffer is the same for all of
    // them; a trajectory that retires stays where it was last written (`where`), and the rows left in the workspace buffer move to
    // the caller's arrays once, at the end.  (ZOPT_AMD_ILQR_SWAP=0: the acceptance step copies, as before; same results.)
    static const bool swap_on = [] {
        const char* e = zm::lab_env("ZOPT_AMD_ILQR_SWAP");
        return !(e && e[0] == '0');
    }();
    double *curX = xTraj, *curU = uTraj, *altX = ws + w.xT2, *altU = ws + w.uT2;
    int it = 0;
    int64_t count = batch;
    for (; it < c.max_iter; ++it) {                                                                      // (:301-303)
        // Every `sync_every` iterations: rebuild the id list on the device and learn how many trajectories are left.  The expansion
        // launch does not wait for that answer: it goes out behind the compaction with the PREVIOUS count (list entries past the new
        // count are ids of the previous list: inactive ones are skipped by the mask, a still-active one is merely expanded twice --
        // the same values into the same rows), and the host round trip (~45 us) passes while it runs.
        // (Measured: a longer interval once the active set is small does not pay -- a stale list costs the DDP tail 1-3 %.)
        const bool sync_now = (it % c.sync_every == 0);
        unsigned seq = 0;
        if (sync_now) {
            seq = lease.next_seq();
            hipLaunchKernelGGL(zm::compact_active_kernel, dim3(1), dim3(1024), 0, st, (const int*)active, (long)batch, (int*)list,
                               (int*)dcount, hword, seq);
            ZM_HIP_CHECK(hipEventRecord(count_ready, st));   // only waited for if the pinned word does not show up (wait_for_count)
        }
        // expansions along the current trajectories: [f_x | f_u], c_x, c_u, v_x in one launch                  (:304-313)
        // (a recorded cost: the model's own expansion with full Jacobians, then the cost's with its per-point Hessians)
        if (ck.traced) {
            rc = zm_linearize_dynamics_list_f64(model, curX, curU, list, count, active, nullptr, ws + w.f_x, ws + w.f_u, batch, T, st);
            if (rc) return rc;
            rc = zm_traced_cost_expand_list_f64(ck.traced, curX, curU, list, count, active, nullptr, ws + w.c_x, ws + w.c_u, ws + w.c_xx,
                                                ws + w.c_ux, ws + w.c_uu, nullptr, ws + w.v_x, ws + w.v_xx, batch, T, st);
        } else {
            rc = zm::expand_list(model, cost, curX, curU, list, count, active, ws + w.f_x, ws + w.f_u, ws + w.c_x, ws + w.c_u,
                                 ws + w.v_x, batch, T, st, plan.packed ? 1 : 0, ck.ref_ptr());
        }
        if (rc) return rc;
        if (sync_now) {
            int32_t c32 = 0;
            rc = zm::wait_for_count(hword, seq, count_ready, dcount, &c32);
            if (rc) return rc;
            count = c32;
            if (count == 0) break;
        }
        if (ck.pen) {   // (behind the round trip: the list and its count are this iteration's)
            rc = zm::state_penalty_expand(ck.pen->sbox, curX, list, count, active, ws + w.c_x, ws + w.v_x, ck.pen->h, ck.pen->visits, batch,
                                          T, n, st);
            if (rc) return rc;
        }
        if (ck.con) {   // (likewise; no projection behind it: the addend is positive semidefinite, the shared set conditioned)
            const zm::ConPen& cp = *ck.con;
            rc = zm::traced_con_expand(cp.tc, curX, curU, list, count, active, cp.sc_xx, cp.sc_ux, cp.sc_uu, cp.sv_xx, ws + w.c_x,
                                       ws + w.c_u, ws + w.v_x, ws + w.c_xx, ws + w.c_ux, ws + w.c_uu, ws + w.v_xx, cp.visits, batch, T, st);
            if (rc) return rc;
        }
        if (ck.traced) {   // the PD projections of the listed trajectories' Hessians, per iteration                 (:312-313)
            rc = zm::condition_cost_listed(ws + w.c_xx, ws + w.c_ux, ws + w.c_uu, (const int*)list, (long)count, T, n, m, 1e-3, st);
            if (rc) return rc;
            rc = zm::psd_project_listed(ws + w.v_xx, (const int*)list, (long)count, n, 1e-3, st);
            if (rc) return rc;
        }
        rc = zm::backward_sweep(plan, ck, model, ws, w, curX, curU, list, count, active, L, batch, T, st);
        if (rc) return rc;
        // 16-way line search (:116-150), then accept: converged = |J - J_new| <= tol, (traj, J) <- (traj_new, J_new) on the listed
        // rows (:316-320)
        if (can_all_store && count <= w.tail_slots) {
            rc = zm::rollout_linesearch_all_store(model, cost, c.x0, ws + w.l, L, curX, curU, ws + w.alphas, list, count, active,
                                                  ws + w.scratch, ws + w.Jn, widx, batch, T, st, ck.ref_ptr());
            if (rc) return rc;
            rc = zm::ilqr_accept(list, count, J, ws + w.Jn, curX, nullptr, curU, nullptr, c.converged, active, c.tol, batch, T, n, m, st,
                                 ws + w.scratch, widx, swap_on ? where : nullptr, curX == xTraj ? 0 : 1);
        } else if (swap_on) {
            rc = zm::cost_linesearch(ck, model, c.x0, ws + w.l, L, curX, curU, ws + w.alphas, 16, list, count, active, altX, altU, ws + w.Jn,
                                     widx, batch, T, st);
            if (rc) return rc;
            rc = zm::ilqr_accept(list, count, J, ws + w.Jn, altX, nullptr, altU, nullptr, c.converged, active, c.tol, batch, T, n, m, st,
                                 nullptr, nullptr, where, altX == xTraj ? 0 : 1);
            std::swap(curX, altX);
            std::swap(curU, altU);
        } else {
            rc = zm::cost_linesearch(ck, model, c.x0, ws + w.l, L, xTraj, uTraj, ws + w.alphas, 16, list, count, active, ws + w.xT2,
                                     ws + w.uT2, ws + w.Jn, widx, batch, T, st);
            if (rc) return rc;
            rc = zm_ilqr_accept_f64(list, count, J, ws + w.Jn, xTraj, ws + w.xT2, uTraj, ws + w.uT2, c.converged, active, c.tol, batch, T,
                                    n, m, st);
        }
        if (rc) return rc;
        // diagnostics (zm_ilqr_solve_trace_f64): row `it` <- every trajectory's cost after this iteration's acceptance step and the
        // line search's winning step-size index (meaningful for the trajectories that were active in this iteration)
        if (c.J_trace) ZM_HIP_CHECK(hipMemcpyAsync(c.J_trace + (long)it * batch, J, sizeof(double) * batch, hipMemcpyDeviceToDevice, st));
        if (c.alpha_trace)
            ZM_HIP_CHECK(hipMemcpyAsync(c.alpha_trace + (long)it * batch, widx, sizeof(int32_t) * batch, hipMemcpyDeviceToDevice, st));
    }
    if (swap_on) {
        rc = zm::ilqr_collect(where, xTraj, ws + w.xT2, uTraj, ws + w.uT2, batch, T, n, m, st);
        if (rc) return rc;
    }
    if (c.iterations) *c.iterations = it;
    return ZM_OK;
}

// The eight entries: each resolves its cost argument(s), fills the record and runs the loop (the state entries: the AL loop around it).
// The plain forms are the trace forms without a trace.
static int solve_entry(SolveCall c, const zm_quadcost_t* cost, const zm_trackcost_t* track, zm::CostArg form, const char* who,
                       const zm_inputbox_t* box = nullptr, int32_t* qp_capped = nullptr) {
    if (c.batch == 0) return ZM_OK;
    if (const int rc = zm::cost_resolve(cost, track, form, who, &c.ck)) return rc;
    c.ck.box = box;
    c.ck.qp_capped = qp_capped;
    return ilqr_solve_impl(c);
}

extern "C" int zm_ilqr_solve_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* uGuess,
                                       int ddp, int max_iter, double tol, int sync_every, double* workspace,
                                       int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                                       int32_t* converged, int32_t* iterations, int64_t batch, int T, void* stream, double* J_trace,
                                       int32_t* alpha_trace) {
    return solve_entry(SolveCall{model, {}, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj,
                                 L, J, converged, iterations, batch, T, stream, J_trace, alpha_trace},
                       cost, nullptr, zm::CostArg::quad, "zm_ilqr_solve_f64");
}

extern "C" int zm_ilqr_solve_f64(const zm_model_t* model, const zm_quadcost_t* cost, const double* x0, const double* uGuess,
                                 int ddp, int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles,
                                 int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J, int32_t* converged,
                                 int32_t* iterations, int64_t batch, int T, void* stream) {
    return zm_ilqr_solve_trace_f64(model, cost, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork, xTraj,
                                   uTraj, L, J, converged, iterations, batch, T, stream, nullptr, nullptr);
}

extern "C" int zm_ilqr_solve_tracking_trace_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* uGuess,
                                                int ddp, int max_iter, double tol, int sync_every, double* workspace,
                                                int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L,
                                                double* J, int32_t* converged, int32_t* iterations, int64_t batch, int T, void* stream,
                                                double* J_trace, int32_t* alpha_trace) {
    return solve_entry(SolveCall{model, {}, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj,
                                 L, J, converged, iterations, batch, T, stream, J_trace, alpha_trace},
                       nullptr, cost, zm::CostArg::track, "zm_ilqr_solve_tracking_f64");
}

extern "C" int zm_ilqr_solve_tracking_f64(const zm_model_t* model, const zm_trackcost_t* cost, const double* x0, const double* uGuess,
                                          int ddp, int max_iter, double tol, int sync_every, double* workspace,
                                          int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                                          int32_t* converged, int32_t* iterations, int64_t batch, int T, void* stream) {
    return zm_ilqr_solve_tracking_trace_f64(model, cost, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork,
                                            xTraj, uTraj, L, J, converged, iterations, batch, T, stream, nullptr, nullptr);
}

// A recorded cost (zm_tracedcost_t; traced_cost.hip): the same loop with the cost's own line search and expansion and per-point Hessians.
extern "C" int64_t zm_traced_cost_solve_workspace_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, int64_t batch, int T, int ddp) {
    if (!model || !tcost || batch < 0 || T < 1) return -1;
    uint32_t mask = 0;
    int32_t npairs = 0;
    if (ddp && (zm_model_nonlinear_mask(model, &mask) != ZM_OK || zm_model_hessian_pairs(model, nullptr, &npairs) != ZM_OK)) return -1;
    return zm::carve(model, batch, T, ddp, (mask >> model->n) != 0, npairs, true).total;
}

extern "C" int zm_traced_cost_solve_trace_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0, const double* uGuess,
                                              int ddp, int max_iter, double tol, int sync_every, double* workspace,
                                              int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J,
                                              int32_t* converged, int32_t* iterations, int64_t batch, int T, void* stream, double* J_trace,
                                              int32_t* alpha_trace) {
    const char* who = "zm_traced_cost_solve_f64";
    if (batch == 0) return ZM_OK;
    if (!model) return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    if (const int rc = zm::tracedcost_check(tcost, who)) return rc;   // (host code: before anything touches the device)
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    if (md.n != tcost->n || md.m != tcost->m)
        return zm::set_error(ZM_EINVAL, "%s: the cost is (n=%d, m=%d), the model (n=%d, m=%d)", who, tcost->n, tcost->m, md.n, md.m);
    SolveCall c{model, {}, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj,
                L, J, converged, iterations, batch, T, stream, J_trace, alpha_trace};
    c.ck.traced = tcost;
    return ilqr_solve_impl(c);
}

extern "C" int zm_traced_cost_solve_f64(const zm_model_t* model, const zm_tracedcost_t* tcost, const double* x0, const double* uGuess, int ddp,
                                        int max_iter, double tol, int sync_every, double* workspace, int64_t workspace_doubles,
                                        int32_t* iwork, double* xTraj, double* uTraj, double* L, double* J, int32_t* converged,
                                        int32_t* iterations, int64_t batch, int T, void* stream) {
    return zm_traced_cost_solve_trace_f64(model, tcost, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork,
                                          xTraj, uTraj, L, J, converged, iterations, batch, T, stream, nullptr, nullptr);
}

// Extension; the reference has no counterpart: the iLQR (ddp = 0) or DDP (ddp = 1) loop with input bounds.
extern "C" int zm_ilqr_solve_box_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                           const zm_inputbox_t* box, const double* x0, const double* uGuess, int ddp, int max_iter,
                                           double tol, int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork,
                                           double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations,
                                           int32_t* qp_capped, int64_t batch, int T, void* stream, double* J_trace,
                                           int32_t* alpha_trace) {
    if (batch != 0 && !box) return zm::set_error(ZM_EINVAL, "zm_ilqr_solve_box_f64: null box");
    return solve_entry(SolveCall{model, {}, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj,
                                 L, J, converged, iterations, batch, T, stream, J_trace, alpha_trace},
                       cost, track, zm::CostArg::exactly_one, "zm_ilqr_solve_box_f64", box, qp_capped);
}

extern "C" int zm_ilqr_solve_box_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                     const zm_inputbox_t* box, const double* x0, const double* uGuess, int ddp, int max_iter, double tol,
                                     int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj,
                                     double* uTraj, double* L, double* J, int32_t* converged, int32_t* iterations, int32_t* qp_capped,
                                     int64_t batch, int T, void* stream) {
    return zm_ilqr_solve_box_trace_f64(model, cost, track, box, x0, uGuess, ddp, max_iter, tol, sync_every, workspace, workspace_doubles,
                                       iwork, xTraj, uTraj, L, J, converged, iterations, qp_capped, batch, T, stream, nullptr, nullptr);
}

// Extension; the reference has no counterpart: iLQR with bounds on the states by an augmented-Lagrangian outer loop around the loop
// above (AL-iLQR).  Host code: per outer iteration one inner solve over the trajectories that are not done, then the multiplier update.
// What the state solve carves behind the inner solve's workspace (offsets in doubles from its start).
struct StateWs {
    int64_t base;       // the inner solve's own workspace (zm_ilqr_solve_workspace_f64, ddp = 0); -1: cannot be sized
    int64_t h;          // (batch, T+1, n) diagonal addend of the cost Hessians
    int64_t Jal;        // (batch) J_AL
    int64_t notdone;    // int32 (batch): the trajectories that are not done
    int64_t remaining;  // int32: how many of them go on
    int64_t total;
    StateWs(const zm_model_t* model, int64_t batch, int T) : base(zm_ilqr_solve_workspace_f64(model, batch, T, 0)) {
        h = base;
        Jal = h + (((int64_t)batch * (T + 1) * (model ? model->n : 0) + 1) & ~(int64_t)1);
        notdone = Jal + ((batch + 1) & ~(int64_t)1);
        remaining = notdone + (batch + 1) / 2;   // (behind the mask: int32 index (batch + 1) & ~1 of its piece)
        total = remaining + 3;
    }
};

// The outer loop of the two augmented-Lagrangian entries (zm_ilqr_solve_state_f64, zm_traced_con_solve_f64): per outer iteration
// `bind(j)` points the call's cost at this iteration's penalty record, the inner solve runs over the trajectories that are not done,
// `update(more)` is the entry's multiplier update (more: another outer iteration may follow), and the host learns how many go on.
struct AlTraces {
    double* J_trace;
    int32_t* alpha_trace;
    double *violation_trace, *mu_trace;
};
template <class Bind, class Update>
static int al_outer_loop(SolveCall& c, int outer, const double* mu, const double* violation, int32_t* remaining, int32_t* iterations,
                         const AlTraces& tr, Bind bind, Update update) {
    hipStream_t st = (hipStream_t)c.stream;
    const int64_t batch = c.batch;
    int ran = 0;
    for (int j = 0; j < outer; ++j) {
        bind(j);
        c.J_trace = tr.J_trace ? tr.J_trace + (long)j * c.max_iter * batch : nullptr;
        c.alpha_trace = tr.alpha_trace ? tr.alpha_trace + (long)j * c.max_iter * batch : nullptr;
        if (tr.mu_trace) ZM_HIP_CHECK(hipMemcpyAsync(tr.mu_trace + (long)j * batch, mu, sizeof(double) * batch, hipMemcpyDeviceToDevice, st));
        int rc = ilqr_solve_impl(c);
        if (rc) return rc;
        ZM_HIP_CHECK(hipMemsetAsync(remaining, 0, sizeof(int32_t), st));
        rc = update(j + 1 < outer ? 1 : 0);
        if (rc) return rc;
        if (tr.violation_trace)
            ZM_HIP_CHECK(hipMemcpyAsync(tr.violation_trace + (long)j * batch, violation, sizeof(double) * batch, hipMemcpyDeviceToDevice, st));
        int32_t left = 0;
        ZM_HIP_CHECK(hipMemcpyAsync(&left, remaining, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        ZM_HIP_CHECK(hipStreamSynchronize(st));
        ran = j + 1;
        if (left == 0) break;
    }
    if (iterations) *iterations = ran;
    return ZM_OK;
}

extern "C" int64_t zm_ilqr_solve_state_workspace_f64(const zm_model_t* model, int64_t batch, int T) {
    const StateWs s(model, batch, T);
    return s.base < 0 ? -1 : s.total;
}

extern "C" int zm_ilqr_solve_state_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                             const zm_inputbox_t* box, const zm_statebox_t* sbox, double mu0, double growth, double mu_max,
                                             int outer, double ctol, const double* x0, const double* uGuess, int ddp, int max_iter,
                                             double tol, int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork,
                                             double* xTraj, double* uTraj, double* L, double* J, int32_t* converged, double* violation,
                                             int32_t* outer_iterations, int32_t* inner_iterations, int32_t* iterations,
                                             int32_t* qp_capped, int64_t batch, int T, void* stream, double* J_trace,
                                             int32_t* alpha_trace, double* violation_trace, double* mu_trace) {
    const char* who = "zm_ilqr_solve_state_f64";
    if (batch == 0) return ZM_OK;
    // every argument is checked here, before the first launch (also what the kernels' own entry points would refuse behind it)
    if (!model || !sbox || !x0 || !uGuess || !workspace || !iwork || !xTraj || !uTraj || !L || !J || !converged || !violation)
        return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    SolveCall c{model, {}, x0, uGuess, 0, max_iter, tol, sync_every, workspace, 0, iwork, xTraj, uTraj, L, nullptr, converged, nullptr,
                batch, T, stream};
    if (const int rc = zm::cost_resolve(cost, track, zm::CostArg::exactly_one, who, &c.ck)) return rc;
    if (ddp != 0) return zm::set_error(ZM_EUNSUPPORTED, "%s: DDP with state bounds is not built (ddp must be 0)", who);
    if (batch < 0 || T < 1 || max_iter < 0 || sync_every < 1) return zm::set_error(ZM_EINVAL, "%s: bad size", who);
    if (!(mu0 > 0.0) || !(growth >= 1.0) || !(mu_max >= mu0) || outer < 1 || !(ctol >= 0.0))
        return zm::set_error(ZM_EINVAL, "%s: need mu0 > 0, growth >= 1, mu_max >= mu0, outer >= 1, ctol >= 0", who);
    const int n = model->n, m = model->m;
    if (n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (state box: n<=12, m<=4)", who, n, m);
    if (const int rc = zm::statebox_check(sbox, n, who)) return rc;
    if (box)
        if (const int rc = zm::box_check_constant(box, m, T, who)) return rc;
    if (cost && (!cost->Q || !cost->R || !cost->Qf)) return zm::set_error(ZM_EINVAL, "%s: cost needs Q, R, Qf", who);
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    if (md.n != n || md.m != m)
        return zm::set_error(ZM_EINVAL, "%s: the %s model is (%d, %d)", who, md.kind == ZM_MODEL_QUADCOPTER ? "quadcopter" : "rigid-body",
                             md.n, md.m);
    if ((int64_t)T * n * n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31)) return zm::set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    const StateWs sw(model, batch, T);
    if (sw.base < 0 || workspace_doubles < sw.total)
        return zm::set_error(ZM_EINVAL, "%s: workspace of %lld doubles, %lld needed", who, (long long)workspace_doubles,
                             (long long)(sw.base < 0 ? -1 : sw.total));
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)batch * (T + 1) * n;
    double* h = workspace + sw.h;
    // the mask of the trajectories that are not done: the inner solve's own `active` mask (iwork) also drops what merely converged
    int32_t* notdone = (int32_t*)(workspace + sw.notdone);
    int32_t* remaining = (int32_t*)(workspace + sw.remaining);
    const unsigned fb = (unsigned)((batch + 255) / 256);
    hipLaunchKernelGGL(zm::fill_i32_kernel, dim3(fb), dim3(256), 0, st, (int*)notdone, (long)batch, 1);
    hipLaunchKernelGGL(zm::fill_f64_kernel, dim3(fb), dim3(256), 0, st, sbox->mu, (long)batch, mu0);
    ZM_HIP_CHECK(hipMemsetAsync(sbox->lam_lb, 0, sizeof(double) * rows, st));
    ZM_HIP_CHECK(hipMemsetAsync(sbox->lam_ub, 0, sizeof(double) * rows, st));
    ZM_HIP_CHECK(hipMemsetAsync(converged, 0, sizeof(int32_t) * batch, st));
    if (outer_iterations) ZM_HIP_CHECK(hipMemsetAsync(outer_iterations, 0, sizeof(int32_t) * batch, st));
    if (inner_iterations) ZM_HIP_CHECK(hipMemsetAsync(inner_iterations, 0, sizeof(int32_t) * batch * outer, st));
    if (box && qp_capped) ZM_HIP_CHECK(hipMemsetAsync(qp_capped, 0, sizeof(int32_t) * batch, st));
    // the inner solves: the loop above on J_AL (written to the workspace; the caller's J receives the cost without the penalty)
    c.workspace_doubles = sw.base;
    c.J = workspace + sw.Jal;
    c.ck.box = box;
    c.ck.qp_capped = box ? qp_capped : nullptr;
    zm::StatePen pen{};
    return al_outer_loop(
        c, outer, sbox->mu, violation, remaining, iterations, AlTraces{J_trace, alpha_trace, violation_trace, mu_trace},
        [&](int j) {
            pen = zm::StatePen{sbox, h, J, inner_iterations ? inner_iterations + (long)j * batch : nullptr, notdone, j == 0 ? uGuess : uTraj};
            c.ck.pen = &pen;
        },
        [&](int update) {
            return zm_state_multiplier_update_f64(sbox, xTraj, notdone, converged, violation, outer_iterations, remaining, ctol, growth,
                                                  mu_max, update, batch, T, n, stream);
        });
}

extern "C" int zm_ilqr_solve_state_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                       const zm_inputbox_t* box, const zm_statebox_t* sbox, double mu0, double growth, double mu_max,
                                       int outer, double ctol, const double* x0, const double* uGuess, int ddp, int max_iter, double tol,
                                       int sync_every, double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj,
                                       double* uTraj, double* L, double* J, int32_t* converged, double* violation,
                                       int32_t* outer_iterations, int32_t* inner_iterations, int32_t* iterations, int32_t* qp_capped,
                                       int64_t batch, int T, void* stream) {
    return zm_ilqr_solve_state_trace_f64(model, cost, track, box, sbox, mu0, growth, mu_max, outer, ctol, x0, uGuess, ddp, max_iter, tol,
                                         sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj, L, J, converged, violation,
                                         outer_iterations, inner_iterations, iterations, qp_capped, batch, T, stream, nullptr, nullptr,
                                         nullptr, nullptr);
}

// Extension; the reference has no counterpart: AL-iLQR on recorded inequality constraints (zm_tracedcon_t; traced_con.hip) -- the outer
// loop of zm_ilqr_solve_state_f64 with the constraint's line search, expansion and multiplier update in place of the state box's.
// What the solve carves behind the inner solve's workspace (offsets in doubles from its start).
struct ConWs {
    int64_t base;       // the inner solve's own workspace with per-point Hessians (zm_traced_cost_solve_workspace_f64's size); -1: cannot
    int64_t sc_xx, sc_ux, sc_uu, sv_xx;   // the shared conditioned Hessians of the quadratic cost
    int64_t Jal;        // (batch) J_AL
    int64_t notdone;    // int32 (batch): the trajectories that are not done
    int64_t remaining;  // int32: how many of them go on
    int64_t total;
    ConWs(const zm_model_t* model, int64_t batch, int T)
        : base((model && batch >= 0 && T >= 1) ? zm::carve(model, batch, T, 0, 0, 0, true).total : -1) {
        const int64_t n = model ? model->n : 0, m = model ? model->m : 0;
        auto even = [](int64_t v) { return (v + 1) & ~(int64_t)1; };
        sc_xx = base;
        sc_ux = sc_xx + even(n * n);
        sc_uu = sc_ux + even(m * n);
        sv_xx = sc_uu + even(m * m);
        Jal = sv_xx + even(n * n);
        notdone = Jal + even(batch);
        remaining = notdone + (batch + 1) / 2;   // (behind the mask: int32 index (batch + 1) & ~1 of its piece)
        total = remaining + 3;
    }
};

extern "C" int64_t zm_traced_con_solve_workspace_f64(const zm_model_t* model, int64_t batch, int T) {
    const ConWs s(model, batch, T);
    return s.base < 0 ? -1 : s.total;
}

extern "C" int zm_traced_con_solve_trace_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                             const zm_tracedcon_t* con, double mu0, double growth, double mu_max, int outer, double ctol,
                                             const double* x0, const double* uGuess, int ddp, int max_iter, double tol, int sync_every,
                                             double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj,
                                             double* L, double* J, int32_t* converged, double* violation, int32_t* outer_iterations,
                                             int32_t* inner_iterations, int32_t* iterations, int64_t batch, int T, void* stream,
                                             double* J_trace, int32_t* alpha_trace, double* violation_trace, double* mu_trace) {
    const char* who = "zm_traced_con_solve_f64";
    if (batch == 0) return ZM_OK;
    // every argument is checked here, before the first launch (also what the kernels' own entry points would refuse behind it)
    if (!model || !con || !x0 || !uGuess || !workspace || !iwork || !xTraj || !uTraj || !L || !J || !converged || !violation)
        return zm::set_error(ZM_EINVAL, "%s: null pointer", who);
    SolveCall c{model, {}, x0, uGuess, 0, max_iter, tol, sync_every, workspace, 0, iwork, xTraj, uTraj, L, nullptr, converged, nullptr,
                batch, T, stream};
    if (const int rc = zm::cost_resolve(cost, track, zm::CostArg::exactly_one, who, &c.ck)) return rc;
    if (ddp != 0) return zm::set_error(ZM_EUNSUPPORTED, "%s: DDP with recorded constraints is not built (ddp must be 0)", who);
    if (batch < 0 || T < 1 || max_iter < 0 || sync_every < 1) return zm::set_error(ZM_EINVAL, "%s: bad size", who);
    if (!(mu0 > 0.0) || !(growth >= 1.0) || !(mu_max >= mu0) || outer < 1 || !(ctol >= 0.0))
        return zm::set_error(ZM_EINVAL, "%s: need mu0 > 0, growth >= 1, mu_max >= mu0, outer >= 1, ctol >= 0", who);
    if (cost && (!cost->Q || !cost->R || !cost->Qf)) return zm::set_error(ZM_EINVAL, "%s: cost needs Q, R, Qf", who);
    zm_model_t md;
    if (const int rc = zm::model_check(model, who, &md)) return rc;
    const int n = md.n, m = md.m;
    if (model->n != n || model->m != m) return zm::set_error(ZM_EINVAL, "%s: the model's kind is (%d, %d)", who, n, m);
    if (n < 1 || n > zm::MAXN || m < 1 || m > zm::MAXM)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: (n=%d, m=%d) not covered (traced constraint: n<=12, m<=4)", who, n, m);
    if (md.kind == ZM_MODEL_TRACED && track)
        return zm::set_error(ZM_EUNSUPPORTED, "%s: a traced model takes a zm_quadcost_t (the tracking cost on the tape interpreter is not "
                                              "built)", who);
    if (const int rc = zm::tracedcon_check(con, n, m, true, who)) return rc;
    if ((int64_t)T * n * n >= (int64_t)1 << 31 || batch >= ((int64_t)1 << 31)) return zm::set_error(ZM_EUNSUPPORTED, "%s: T*n*n or batch too large", who);
    const ConWs sw(model, batch, T);
    if (sw.base < 0 || workspace_doubles < sw.total)
        return zm::set_error(ZM_EINVAL, "%s: workspace of %lld doubles, %lld needed", who, (long long)workspace_doubles,
                             (long long)(sw.base < 0 ? -1 : sw.total));
    hipStream_t st = (hipStream_t)stream;
    // the mask of the trajectories that are not done: the inner solve's own `active` mask (iwork) also drops what merely converged
    int32_t* notdone = (int32_t*)(workspace + sw.notdone);
    int32_t* remaining = (int32_t*)(workspace + sw.remaining);
    const unsigned fb = (unsigned)((batch + 255) / 256);
    hipLaunchKernelGGL(zm::fill_i32_kernel, dim3(fb), dim3(256), 0, st, (int*)notdone, (long)batch, 1);
    hipLaunchKernelGGL(zm::fill_f64_kernel, dim3(fb), dim3(256), 0, st, con->mu, (long)batch, mu0);
    if (con->n_con > 0) ZM_HIP_CHECK(hipMemsetAsync(con->lam, 0, sizeof(double) * batch * T * con->n_con, st));
    if (con->n_con_terminal > 0) ZM_HIP_CHECK(hipMemsetAsync(con->lam_terminal, 0, sizeof(double) * batch * con->n_con_terminal, st));
    ZM_HIP_CHECK(hipMemsetAsync(converged, 0, sizeof(int32_t) * batch, st));
    if (outer_iterations) ZM_HIP_CHECK(hipMemsetAsync(outer_iterations, 0, sizeof(int32_t) * batch, st));
    if (inner_iterations) ZM_HIP_CHECK(hipMemsetAsync(inner_iterations, 0, sizeof(int32_t) * batch * outer, st));
    // the inner solves: the loop above on J_AL (written to the workspace; the caller's J receives the cost without the penalty)
    c.workspace_doubles = sw.base;
    c.J = workspace + sw.Jal;
    zm::ConPen pen{};
    return al_outer_loop(
        c, outer, con->mu, violation, remaining, iterations, AlTraces{J_trace, alpha_trace, violation_trace, mu_trace},
        [&](int j) {
            pen = zm::ConPen{con, workspace + sw.sc_xx, workspace + sw.sc_ux, workspace + sw.sc_uu, workspace + sw.sv_xx, J,
                             inner_iterations ? inner_iterations + (long)j * batch : nullptr, notdone, j == 0 ? uGuess : uTraj};
            c.ck.con = &pen;
        },
        [&](int update) {
            return zm_traced_con_multiplier_update_f64(con, xTraj, uTraj, notdone, converged, violation, outer_iterations, remaining, ctol,
                                                       growth, mu_max, update, batch, T, stream);
        });
}

extern "C" int zm_traced_con_solve_f64(const zm_model_t* model, const zm_quadcost_t* cost, const zm_trackcost_t* track,
                                       const zm_tracedcon_t* con, double mu0, double growth, double mu_max, int outer, double ctol,
                                       const double* x0, const double* uGuess, int ddp, int max_iter, double tol, int sync_every,
                                       double* workspace, int64_t workspace_doubles, int32_t* iwork, double* xTraj, double* uTraj, double* L,
                                       double* J, int32_t* converged, double* violation, int32_t* outer_iterations,
                                       int32_t* inner_iterations, int32_t* iterations, int64_t batch, int T, void* stream) {
    return zm_traced_con_solve_trace_f64(model, cost, track, con, mu0, growth, mu_max, outer, ctol, x0, uGuess, ddp, max_iter, tol,
                                         sync_every, workspace, workspace_doubles, iwork, xTraj, uTraj, L, J, converged, violation,
                                         outer_iterations, inner_iterations, iterations, batch, T, stream, nullptr, nullptr, nullptr,
                                         nullptr);
}

extern "C" int zm_shutdown(void) { return zm::release_host_slots(); }
