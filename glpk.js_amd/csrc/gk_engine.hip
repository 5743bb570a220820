// libglpk_mi355x host side: the C-ABI of include/glpk_mi355x.h.
//
// The control flow of spx_primal / spx_dual (glpspx01.js:1705-2056,
// glpspx02.js:1614-1966) runs here unchanged; the inner "normal pivot" path
// of each loop is executed on the device in batches (gk_kernels.hip), and
// the host only resumes at the branch the device stopped on (DState.stop).
// Problem data, the basis header and the explicit inverse stay resident in
// HBM across calls; O(m+n) vectors cross PCIe only at phase switches,
// refactorizations and store_sol.
#include "gk_device.h"
#include "../../include/glpk_mi355x.h"

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace gk;

namespace {

thread_local std::string g_err;

void set_err(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

struct AbiError {
    std::string msg;
};

#define HIPCHK(x)                                                                            \
    do {                                                                                     \
        hipError_t e__ = (x);                                                                \
        if (e__ != hipSuccess) throw AbiError{std::string("HIP error ") + hipGetErrorString(e__) + " at " #x}; \
    } while (0)

#define ABI_REQUIRE(c, ...)                                                                  \
    do {                                                                                     \
        if (!(c)) {                                                                          \
            char b__[512];                                                                   \
            snprintf(b__, sizeof b__, __VA_ARGS__);                                          \
            throw AbiError{b__};                                                             \
        }                                                                                    \
    } while (0)

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <typename T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    bool own = true;                      // false: a view into an arena (Engine::arena)
    void ensure(size_t cnt)
    {
        if (cnt <= n && p) return;
        if (p && own) (void)hipFree(p);
        p = nullptr;
        n = 0;
        own = true;
        size_t bytes = std::max<size_t>(cnt, 1) * sizeof(T);
        HIPCHK(hipMalloc((void **)&p, bytes));
        n = std::max<size_t>(cnt, 1);
    }
    void view(T *q, size_t cnt)
    {
        if (p && own) (void)hipFree(p);
        p = q;
        n = cnt;
        own = false;
    }
    void release()
    {
        if (p && own) (void)hipFree(p);
        p = nullptr;
        n = 0;
        own = true;
    }
};

}  // namespace

struct gk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int wall_khz = 100000;              // device wall clock (wall_clock64) rate
    // the owner's reference plus one per factor handle: a host whose
    // finalizers run in any order (N-API at exit, Python's GC) may destroy
    // the context before its factors, which still need it
    int refs = 1;
    // scratch every engine on this context borrows (one stream: never used
    // by two solves at once): split-K partials, A w partials, the device side
    // of the staged uploads.  Owned here, so an engine (one per LP object)
    // neither allocates nor frees tens of MiB — freeing them per engine
    // while the process ran was followed by a fault in node's teardown
    DBuf<double> partial, awpart;
    DBuf<char> upstage;
    // the branch-and-bound driver's buffers, kept across searches (gk_mip.hip)
    void *mip_cache = nullptr;
    void (*mip_cache_free)(void *) = nullptr;
    // the look-ahead streams of large re-inversions (gk_reinvert.hip)
    GjSide *gj = nullptr;
    bool gj_tried = false;
    // the branch-and-bound driver's progress lines (gk_ios_set_report)
    gk_report_fn ios_rpt = nullptr;
    void *ios_rpt_ud = nullptr;
};

static void ctx_unref(gk_ctx *ctx)
{
    if (--ctx->refs > 0) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->partial.release(); ctx->awpart.release(); ctx->upstage.release();
    if (ctx->gj) gj_side_destroy(ctx->gj);
    ctx->gj = nullptr;
    if (ctx->mip_cache && ctx->mip_cache_free) ctx->mip_cache_free(ctx->mip_cache);
    ctx->mip_cache = nullptr;
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// a captured device batch of dual pivots: replayed while the device
// pointers, the launch plan and the batch length are unchanged
struct GraphEntry {
    SpxDev d;
    DualPlan pl;
    int K = 0;
    int kind = 0;                               // 0: dual, 1: primal
    hipGraphExec_t exec = nullptr;
    unsigned long long last = 0;
};

// device copy of the problem (A in scaled form) plus the simplex working set
struct Engine {
    int m = 0, n = 0, nnz = 0;
    int dense = 0, lda = 0;
    std::vector<int> hcptr, hcind;            // host copy of the scaled CSC (sparse A: the basis factor is built from it)
    std::vector<double> hcval;
    unsigned long long a_version = 0;
    DBuf<double> A, AT;                     // dense column-major and row-major
    int ldt = 0;
    DBuf<int> cptr, cind, rptr, rcol;        // CSC / CSR
    DBuf<int> lrow;                          // CSR rows longer than CSR_LONG
    int nlr = 0;
    DBuf<double> cval, rval;
    // working set
    DBuf<signed char> type, orig_type, stat, refsp;
    DBuf<double> lb, ub, coef, orig_lb, orig_ub, obj;
    DBuf<int> head, bind;
    DBuf<double> bbar, cbar, gamma, tcol, trow, rho, rowp, u, s, h, wcol, ys, work, r1, r2, partial;
    DBuf<DState> st;
    DBuf<DState> stm;                       // the epilogue's copy of st, in front of the pull region
    DBuf<int> eflags;                       // the epilogue's phase-I check_stab / check_feas results
    DState *st_host = nullptr;              // pinned staging copy of st (hipHostMalloc)
    char *pin = nullptr;                     // pinned staging of the per-call host <-> device copies
    size_t pin_cap = 0;
    DBuf<int> rlist, rpos, rho_idx, wlist, wpos, awcnt;
    DBuf<double> rho_val, gpart, cand, awpart;
    DBuf<char> upstage;                         // device side of the coalesced uploads
    DBuf<int> xlist;                            // eval_cbar: basic slacks with a nonzero cost (primal phase I)
    DBuf<unsigned long long> tslots, xslots;
    DBuf<unsigned long long> dethash;           // GK_DET_LOG fingerprints
    // MFMA pricing panel (gk_panel.hip), dense A only, sized for PANEL_MAX rows
    DBuf<double> pnl, pnl_src;
    DBuf<int> pslot, ppos;
    int pnl_m = -1, pnl_n = -1;
    // the next call's phase-I basic values, evaluated at the end of a dual
    // call stopped by it_lim / tm_lim in phase I (Spx::next_aux_launch): the
    // auxiliary bounds and statuses that call's set_aux_bnds will derive from
    // the same reduced costs, and the eval_bbar result under them
    DBuf<double> lb_n, ub_n, bbar_n;
    DBuf<signed char> stat_n;
    struct NextAux {
        bool ok = false;
        unsigned long long fact_ver = 0;
        std::vector<signed char> stat_var;    // the status by variable (1..m+n) it was evaluated with
    } next_aux;
    hipEvent_t epi_ev = nullptr;              // the end-of-call epilogue's results are on the host (Spx::epi_arm)
    std::vector<GraphEntry> graphs;
    unsigned long long graph_clock = 0;
    int kbatch = 8;                           // batch length carried across calls
    int prof = 0;                             // gk_bfd_profile: events around the pivot-row kernel (2: + block trace)
    std::vector<hipEvent_t> ev;               // 2 per pivot of the longest batch
    DBuf<unsigned long long> trace;           // prof == 2: per-kernel, per-block clock stamps of the last pivot
    // one allocation for the whole O(m + n) working set (the vectors, lists,
    // candidates and the state): a pivot kernel touches tens of these arrays,
    // and one allocation keeps them on a few large pages — as separate
    // allocations each first touch from a CU was a translation miss (the
    // bookkeeping wave of k_dual_update spent 2 us on ten stores)
    char *arena = nullptr;
    size_t arena_cap = 0;
    int arena_m = -1, arena_n = -1;
    // the working set a gk_spx_* call left on the device (host mirrors of it),
    // so that the next call on the same problem — a run of it_lim-bounded
    // calls, or glp_simplex after glp_simplex — does not upload it again and
    // does not repeat an evaluation whose result is already resident
    // (Spx::resident_match); ok is cleared by every call and set again by a
    // normal return
    struct Resident {
        bool ok = false;
        int dual = -1, m = 0, n = 0, nr = 0;
        unsigned long long a_version = 0, fact_ver = 0, b_version = 0;
        int dir = 0;
        double c0 = 0.0;
        double zeta = 0.0;
        std::vector<signed char> type, orig_type, stat;
        std::vector<double> lb, ub, coef, orig_lb, orig_ub, obj, bbar, cbar;
        std::vector<int> head, bind;
        bool cbar_ok = false, bbar_ok = false;
    } res;
    // host mirror vectors of the last call, kept for their capacity: a call
    // assigns into them instead of allocating (and page-faulting) ~20 arrays
    // of m + n entries each time
    struct Spare {
        std::vector<signed char> type, orig_type, stat;
        std::vector<double> lb, ub, coef, orig_lb, orig_ub, obj, bbar, cbar, gamma;
        std::vector<int> head, bind;
    } spare;
    // the auxiliary types and bounds of set_aux_bnds (a function of orig_type
    // alone), kept across calls with the same bounds version; Spx swaps them
    // with its current arrays instead of rebuilding (Spx::set_aux_bnds)
    struct AuxCache {
        bool ok = false;
        std::vector<signed char> type;
        std::vector<double> lb, ub;
    } auxc;
    MatDev mat() const
    {
        MatDev M{};
        M.m = m; M.n = n; M.nnz = nnz; M.dense = dense;
        M.A = A.p; M.lda = lda;
        M.cptr = cptr.p; M.cind = cind.p; M.cval = cval.p;
        M.rptr = rptr.p; M.rcol = rcol.p; M.rval = rval.p;
        M.lrow = lrow.p; M.nlr = dense ? 0 : nlr;
        M.AT = dense ? AT.p : nullptr; M.ldt = ldt;
        int avg = n > 0 ? nnz / n : 0;
        M.lpc = avg >= 48 ? 64 : (avg >= 6 ? 8 : 1);
        return M;
    }
    ~Engine()
    {
        // the captured graphs first: their kernel nodes refer to the buffers
        // below, and an exec destroyed after them (or left to the runtime's
        // own teardown) touches freed allocations
        for (auto &g : graphs)
            if (g.exec) (void)hipGraphExecDestroy(g.exec);
        graphs.clear();
        for (auto e : ev) (void)hipEventDestroy(e);
        ev.clear();
        if (epi_ev) (void)hipEventDestroy(epi_ev);
        A.release(); AT.release(); cptr.release(); cind.release(); rptr.release(); rcol.release(); cval.release(); rval.release();
        rlist.release(); rpos.release(); rho_idx.release(); rho_val.release();
        gpart.release(); awcnt.release(); tslots.release(); xslots.release(); trace.release(); wlist.release(); wpos.release(); cand.release();
        awpart.release();
        pnl.release(); pnl_src.release(); pslot.release(); ppos.release();
        lb_n.release(); ub_n.release(); bbar_n.release(); stat_n.release();
        type.release(); orig_type.release(); stat.release(); refsp.release();
        lb.release(); ub.release(); coef.release(); orig_lb.release(); orig_ub.release(); obj.release();
        head.release(); bind.release();
        bbar.release(); cbar.release(); gamma.release(); tcol.release(); trow.release(); rho.release(); rowp.release();
        u.release(); s.release(); h.release(); wcol.release(); ys.release(); work.release(); r1.release(); r2.release();
        partial.release();
        st.release();
        if (arena) (void)hipFree(arena);
        if (st_host) (void)hipHostFree(st_host);
        if (pin) (void)hipHostFree(pin);
        upstage.release(); xlist.release(); dethash.release();
    }
};

struct gk_bfd {
    gk_ctx *ctx = nullptr;
    gk_bfcp parm{};
    int valid = 0;
    int m = 0, ldb = 0;
    int upd_cnt = 0;
    // product-form updates between re-inversions chosen by the engine (nfs_max
    // left at its default): adapted to the reduced-cost / primal drift measured
    // at every re-inversion (Spx::drift_adapt); 0 = not set yet
    int upd_lim_adapt = 0;
    int clean_runs = 0;                   // consecutive drift measurements below tol / 200
    bool parm_default = true;             // no glp_set_bfcp: the interval is the engine's (gk_bfd_reset_parm)
    unsigned long long fact_ver = 0;           // bumped whenever inv(B) is rebuilt or updated outside a solve
    int ext_upd = 0;                           // updated through gk_bfd_update since the last re-inversion
    int prof = 0;                              // gk_bfd_profile
    DBuf<double> Binv;
    // re-inversion scratch
    DBuf<double> C, X, Y, CinvR, BS, G, vecx, vecy, partial;
    DBuf<int> idx_i, piv_step, piv, flag;
    DBuf<unsigned long long> nwt_bits;         // max |I - C X| of a Newton step (gk_newton.hip)
    DBuf<int> bptr, brow;                      // basis given as CSC (gk_bfd_factorize*)
    DBuf<double> bval;
    Engine *eng = nullptr;
    // the sparse factor (gk_sparse.hip) in place of the explicit inverse:
    // large sparse LPs (m > 65535, or GK_SPARSE=1), dual simplex
    SpFactor *sp = nullptr;
    int sparse = 0;
    gk_spx_stats stats{};
    gk_report_fn rpt = nullptr;                // progress / termination reports (gk_bfd_set_report)
    void *rpt_ud = nullptr;
    LpShard *shard = nullptr;                  // column-sharded pricing (gk_bfd_set_comm), or nullptr
};

// updates the factor takes before it is rebuilt: nfs_max Forrest-Tomlin
// updates (glpfhv.js:182), or nrs_max Schur-complement updates for BG / GR
// (lpf_update_it's LPF_ELIMIT, glplpf.js:359)
static int upd_limit_parm(const gk_bfcp &p)
{
    const int v = (p.type == 2 || p.type == 3) ? p.nrs_max : p.nfs_max;
    return v > 0 ? v : 100;
}

static const size_t PARTIAL_CAP = (size_t)1 << 22;   // >= splits * rows of every gemv (see gemv_plan, dual_plan)
static const int AW_SPLITS = 64;                      // splits of A w over the reference-space columns

// ---------------------------------------------------------------------------
// re-inversion of the basis matrix
// ---------------------------------------------------------------------------
// Basis columns: slack-like unit columns e_r (+1) and "structural" columns.
// With S the rows covered by slack columns (positions posS), R the other
// rows and J the structural positions, C = B[R, J] is k x k and
//   inv(B)[J, R] = inv(C),  inv(B)[posS(s), s] = 1,  inv(B)[posS, R] = -B[S, J] inv(C).
struct BasisSplit {
    int k = 0, ms = 0;
    std::vector<int> posJ, colJ, rowR, posS, rowS, rowmap;   // rowmap[r-1] = a (R) or -(s+1) (S)
};

// refine: inv(B) currently holds the product-form-updated inverse of exactly
// this basis (the engine's scheduled re-inversion): the structural block may
// be re-inverted by Newton refinement on the matrix cores (gk_newton.hip)
static int reinvert_core(gk_bfd *f, const BasisSplit &bs, const MatDev *Adense, int from_csc, double sign,
                         const int *csc_ptr, const int *csc_row, const double *csc_val, bool refine = false)
{
    hipStream_t s = f->ctx->stream;
    const int m = f->m, k = bs.k, ms = bs.ms;
    const double t0 = now_s();
    f->Binv.ensure((size_t)f->ldb * m);
    // index lists on the device: posJ | colJ | rowR | posS | rowS | rowmap
    std::vector<int> packed;
    packed.reserve((size_t)3 * k + 2 * ms + m);
    packed.insert(packed.end(), bs.posJ.begin(), bs.posJ.end());
    packed.insert(packed.end(), bs.colJ.begin(), bs.colJ.end());
    packed.insert(packed.end(), bs.rowR.begin(), bs.rowR.end());
    packed.insert(packed.end(), bs.posS.begin(), bs.posS.end());
    packed.insert(packed.end(), bs.rowS.begin(), bs.rowS.end());
    packed.insert(packed.end(), bs.rowmap.begin(), bs.rowmap.end());
    f->idx_i.ensure(packed.size() + 1);
    HIPCHK(hipMemcpyAsync(f->idx_i.p, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, s));
    int *d_posJ = f->idx_i.p, *d_colJ = d_posJ + k, *d_rowR = d_colJ + k, *d_posS = d_rowR + k,
        *d_rowS = d_posS + ms, *d_rowmap = d_rowS + ms;
    double *result = nullptr;
    if (k > 0) {
        f->C.ensure((size_t)k * k);
        f->X.ensure((size_t)2 * k * k);
        f->Y.ensure(std::max((size_t)2 * k * k, gj_blocked_scratch(k)));
        f->CinvR.ensure((size_t)k * k);
        if (ms > 0) {
            f->BS.ensure((size_t)ms * k);
            f->G.ensure((size_t)ms * k);
        }
        if (from_csc) {
            // C and BS from CSC columns (sign applied), selected by colJ
            fill_d(s, f->X.p, 0.0, (size_t)k * k);
            if (ms > 0) fill_d(s, f->BS.p, 0.0, (size_t)ms * k);
            extern void gather_csc_sel(hipStream_t, int, const int *, const int *, const int *, const double *,
                                       const int *, double *, double *, int, double);
            gather_csc_sel(s, k, d_colJ, csc_ptr, csc_row, csc_val, d_rowmap, f->X.p, f->BS.p, ms, sign);
        } else {
            gather_basis_blocks(s, *Adense, m, k, d_colJ, d_rowR, f->X.p, f->BS.p, ms, d_rowS);
        }
        const double *cinv = nullptr;
        if (refine && f->valid && !f->ext_upd && newton_min_k() > 0 && k >= newton_min_k()) {
            f->nwt_bits.ensure(1);
            NewtonInfo ni;
            // C sits in the first k^2 of X; the second half holds the
            // column-major copy of the iterate
            cinv = newton_refine(s, k, f->X.p, f->Binv.p, f->ldb, d_posJ, d_rowR, f->CinvR.p, f->Y.p,
                                 f->Y.p + (size_t)k * k, f->X.p + (size_t)k * k, f->nwt_bits.p, &ni);
            f->stats.refine_tries++;
            f->stats.refine_resid_max = std::max(f->stats.refine_resid_max, ni.resid);
            if (cinv) {
                f->stats.refinements++;
                f->stats.refine_steps += ni.steps;
            }
        }
        if (cinv) {
            if (ms > 0) gemm_bs_cinv(s, f->BS.p, ms, k, cinv, f->G.p, 1);
            assemble_binv(s, f->Binv.p, m, f->ldb, k, ms, d_posJ, d_rowR, d_posS, d_rowS, cinv, f->G.p);
            HIPCHK(hipStreamSynchronize(s));
            f->fact_ver++;
            f->valid = 1;
            f->upd_cnt = 0;
            f->ext_upd = 0;
            f->stats.reinversions++;
            f->stats.seconds_reinvert += now_s() - t0;
            return 0;
        }
        f->piv_step.ensure(k);
        f->piv.ensure(k);
        f->flag.ensure(1);
        const bool blocked = k <= gj_blocked_max();
        // GK_GJ_TIME=1 (tools/prof_reinvert.py): device span of the
        // Gauss–Jordan inversion by events on s, printed to stderr
        static const bool gj_time = std::getenv("GK_GJ_TIME") != nullptr;
        hipEvent_t gj_ev[2] = {nullptr, nullptr};
        if (gj_time) {
            HIPCHK(hipEventCreate(&gj_ev[0]));
            HIPCHK(hipEventCreate(&gj_ev[1]));
            HIPCHK(hipEventRecord(gj_ev[0], s));
        }
        GjSide *side = nullptr;
        if (blocked && gj_lookahead(k)) {
            if (!f->ctx->gj && !f->ctx->gj_tried) {
                f->ctx->gj_tried = true;
                f->ctx->gj = gj_side_create(f->ctx->device);
            }
            side = f->ctx->gj;
        }
        if (blocked)
            result = gauss_jordan_blocked(s, f->X.p, f->Y.p, k, f->piv_step.p, f->piv.p, f->flag.p, 1e-15, side);
        else gauss_jordan(s, f->X.p, f->Y.p, k, f->piv_step.p, f->piv.p, f->flag.p, 1e-15, &result);
        if (gj_time) {
            float ms = 0.f;
            HIPCHK(hipEventRecord(gj_ev[1], s));
            HIPCHK(hipEventSynchronize(gj_ev[1]));
            HIPCHK(hipEventElapsedTime(&ms, gj_ev[0], gj_ev[1]));
            fprintf(stderr, "gauss-jordan k=%d: %.3f ms (device, events)\n", k, ms);
            (void)hipEventDestroy(gj_ev[0]);
            (void)hipEventDestroy(gj_ev[1]);
        }
        int flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, f->flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (flag) {
            f->fact_ver++;
            f->valid = 0;
            f->stats.reinversions++;
            f->stats.seconds_reinvert += now_s() - t0;
            return 1;   // BFD_ESING
        }
        if (blocked) extract_inverse_blocked(s, result, k, f->piv.p, f->piv_step.p, f->CinvR.p);
        else extract_inverse_rowmajor(s, result, k, f->piv.p, f->CinvR.p);
        if (ms > 0) gemm_bs_cinv(s, f->BS.p, ms, k, f->CinvR.p, f->G.p, 1);
    }
    assemble_binv(s, f->Binv.p, m, f->ldb, k, ms, d_posJ, d_rowR, d_posS, d_rowS, f->CinvR.p, f->G.p);
    HIPCHK(hipStreamSynchronize(s));
    f->fact_ver++;
    f->valid = 1;
    f->upd_cnt = 0;
    f->ext_upd = 0;
    f->stats.reinversions++;
    f->stats.seconds_reinvert += now_s() - t0;
    return 0;
}

// split by the basis header of (I | -A): head[1..m] (1-based values)
static bool split_from_head(int m, const int *head1, BasisSplit &bs)
{
    bs = BasisSplit();
    std::vector<int> srow_pos(m + 1, 0);
    for (int i = 1; i <= m; i++) {
        int k = head1[i];
        if (k <= m) {
            if (srow_pos[k]) return false;
            srow_pos[k] = i;
        } else {
            bs.posJ.push_back(i);
            bs.colJ.push_back(k - m);
        }
    }
    bs.rowmap.assign(m, 0);
    for (int r = 1; r <= m; r++) {
        if (srow_pos[r]) {
            bs.rowmap[r - 1] = -(int)(bs.rowS.size() + 1);
            bs.rowS.push_back(r);
            bs.posS.push_back(srow_pos[r]);
        } else {
            bs.rowmap[r - 1] = (int)bs.rowR.size();
            bs.rowR.push_back(r);
        }
    }
    bs.k = (int)bs.posJ.size();
    bs.ms = (int)bs.rowS.size();
    return bs.k == (int)bs.rowR.size();
}

// ---------------------------------------------------------------------------
// device working set
// ---------------------------------------------------------------------------
static void engine_alloc(Engine &E, int m, int n, gk_ctx *ctx)
{
    const size_t mn = (size_t)m + n;
    const size_t gv = (size_t)(std::max(m, n) + 255) / 256 + 1;
    if (E.arena_m != m || E.arena_n != n) {
        // the working set as views into one arena (256-byte aligned slices)
        size_t off = 0;
        char *base = nullptr;
        auto place = [&](auto &b, size_t cnt) {
            using T = typename std::remove_pointer<decltype(b.p)>::type;
            cnt = std::max<size_t>(cnt, 1);
            if (base) b.view((T *)(base + off), cnt);
            off += (cnt * sizeof(T) + 255) & ~(size_t)255;
        };
        auto layout = [&]() {
            off = 0;
            place(E.st, 1);
            place(E.type, mn); place(E.orig_type, mn); place(E.refsp, mn);
            place(E.lb, mn); place(E.ub, mn); place(E.orig_lb, mn); place(E.orig_ub, mn);
            place(E.obj, n);
            // what pull() brings back, contiguous: one copy (the epilogue's
            // download starts at its copy of the state and check flags)
            place(E.stm, 1); place(E.eflags, 2 * ((mn + 255) / 256) + 4);
            place(E.head, mn); place(E.bind, mn); place(E.stat, n); place(E.bbar, m); place(E.cbar, n);
            place(E.coef, mn);
            place(E.gamma, std::max(m, n));
            place(E.tcol, m); place(E.trow, n); place(E.rho, m); place(E.rowp, m); place(E.u, m); place(E.s, n);
            place(E.h, m); place(E.wcol, n); place(E.ys, m); place(E.work, std::max(m, n)); place(E.r1, m);
            place(E.r2, m);
            // + a spare slot each (branch-free list updates, books_store)
            place(E.rlist, (size_t)m + 1); place(E.rpos, (size_t)m + 1);
            place(E.rho_idx, (size_t)m + 1); place(E.rho_val, (size_t)m + 1);
            // dual: gamma_p sums, then per-block max |trow| (64-slot blocks), 4
            // gv each; primal: max |tcol|, d_q sums, gamma_q sums of the row
            // groups, 16 gv each
            place(E.gpart, 56 * gv);
            // candidates (24-byte entries): chuzr (4 gv, or one per 16 rows
            // for k_dual_update: cand_chuzr_cap) | pass 1 | pass 2, 4 gv each,
            // then the primal pass-1 candidates of the row groups, 16 gv
            place(E.cand, 3 * (28 * gv + ((size_t)m + 15) / 16));
            // dual: reference-space non-basic structurals (n); primal: basic
            // slacks in the reference space (m)
            place(E.wlist, (size_t)std::max(m, n) + 1); place(E.wpos, (size_t)std::max(m, n) + 1);
            place(E.awcnt, (size_t)(m + 511) / 512 + 1);
            place(E.tslots, std::max((size_t)((n + 511) / 512) * 2048, 4 * gv) + 1);
            place(E.xslots, (size_t)(m + 15) / 16 + gv + (size_t)((m + 511) / 512) * 2048 + 1);
        };
        layout();
        if (E.arena_cap < off) {
            if (E.arena) (void)hipFree(E.arena);
            E.arena = nullptr;
            E.arena_cap = 0;
            HIPCHK(hipMalloc((void **)&E.arena, off));
            E.arena_cap = off;
        }
        base = E.arena;
        layout();
        // arrival counters (reset by their users) and exit stamps start at 0
        HIPCHK(hipMemset(E.awcnt.p, 0, E.awcnt.n * sizeof(int)));
        HIPCHK(hipMemset(E.xslots.p, 0, E.xslots.n * sizeof(unsigned long long)));
        E.arena_m = m;
        E.arena_n = n;
    }
    // the context's scratch (sized once for every m <= 65535)
    ctx->partial.ensure(PARTIAL_CAP);
    ctx->awpart.ensure((size_t)AW_SPLITS * 65536);
    E.partial.view(ctx->partial.p, ctx->partial.n);
    E.awpart.view(ctx->awpart.p, ctx->awpart.n);
    if (!E.st_host) HIPCHK(hipHostMalloc((void **)&E.st_host, sizeof(DState), hipHostMallocDefault));
    {
        const size_t need = std::max<size_t>((size_t)8 << 20, (size_t)32 * ((size_t)m + n + 1) * sizeof(double));
        if (E.pin_cap < need) {
            if (E.pin) (void)hipHostFree(E.pin);
            E.pin = nullptr;
            E.pin_cap = 0;
            HIPCHK(hipHostMalloc((void **)&E.pin, need, hipHostMallocDefault));
            E.pin_cap = need;
        }
    }
}

__global__ void k_densify(const int *cptr, const int *cind, const double *cval, int n, double *A, int lda)
{
    const int c = blockIdx.x;
    if (c >= n) return;
    for (int t = cptr[c] + threadIdx.x; t < cptr[c + 1]; t += blockDim.x) A[(size_t)c * lda + cind[t]] = cval[t];
}

// A := rii * a * sjj as init_csa (glpspx01.js:96-105), uploaded once per a_version
static void engine_upload_matrix(gk_bfd *f, const gk_lp *lp)
{
    Engine &E = *f->eng;
    hipStream_t s = f->ctx->stream;
    const int m = lp->m, n = lp->n, nnz = lp->nnz;
    if (lp->a_version != 0 && lp->a_version == E.a_version && E.m == m && E.n == n && E.nnz == nnz) return;
    E.m = m; E.n = n; E.nnz = nnz;
    std::vector<int> cptr(n + 1), cind(std::max(nnz, 1));
    std::vector<double> cval(std::max(nnz, 1));
    int t = 0;
    for (int j = 1; j <= n; j++) {
        cptr[j - 1] = t;
        for (int p = lp->A_ptr[j]; p < lp->A_ptr[j + 1]; p++) {
            int i = lp->A_ind[p];
            ABI_REQUIRE(1 <= i && i <= m, "gk_spx: A_ind[%d] = %d; row number out of range", p, i);
            cind[t] = i - 1;
            cval[t] = lp->rii[i] * lp->A_val[p] * lp->sjj[j];
            t++;
        }
    }
    cptr[n] = t;
    ABI_REQUIRE(t == nnz, "gk_spx: A_ptr describes %d entries, nnz = %d", t, nnz);
    E.dense = ((double)nnz >= 0.5 * (double)m * (double)n) ? 1 : 0;
    if (!E.dense) {
        E.hcptr = cptr;
        E.hcind = cind;
        E.hcval = cval;
    } else {
        E.hcptr.clear(); E.hcind.clear(); E.hcval.clear();
    }
    E.cptr.ensure(n + 1);
    E.cind.ensure(std::max(nnz, 1));
    E.cval.ensure(std::max(nnz, 1));
    HIPCHK(hipMemcpyAsync(E.cptr.p, cptr.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(E.cind.p, cind.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(E.cval.p, cval.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, s));
    if (E.dense) {
        E.lda = (m + 7) & ~7;
        E.A.ensure((size_t)E.lda * n);
        fill_d(s, E.A.p, 0.0, (size_t)E.lda * n);
        hipLaunchKernelGGL(k_densify, dim3(n), dim3(256), 0, s, E.cptr.p, E.cind.p, E.cval.p, n, E.A.p, E.lda);
        E.ldt = (n + 7) & ~7;
        E.AT.ensure((size_t)E.ldt * m);
        transpose_dense(s, E.A.p, m, n, E.lda, E.AT.p, E.ldt);
    } else {
        // CSR copy (row order of entries does not matter numerically)
        std::vector<int> rptr(m + 1, 0), rcol(std::max(nnz, 1));
        std::vector<double> rval(std::max(nnz, 1));
        for (int q = 0; q < nnz; q++) rptr[cind[q] + 1]++;
        for (int r = 0; r < m; r++) rptr[r + 1] += rptr[r];
        std::vector<int> fillp(rptr.begin(), rptr.end() - 1);
        for (int c = 0; c < n; c++)
            for (int q = cptr[c]; q < cptr[c + 1]; q++) {
                int pos = fillp[cind[q]]++;
                rcol[pos] = c;
                rval[pos] = cval[q];
            }
        E.rptr.ensure(m + 1);
        E.rcol.ensure(std::max(nnz, 1));
        E.rval.ensure(std::max(nnz, 1));
        HIPCHK(hipMemcpyAsync(E.rptr.p, rptr.data(), (m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(E.rcol.p, rcol.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(E.rval.p, rval.data(), (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, s));
        // the long rows (linking rows of a block-angular LP) get a block
        // each in k_dual_ratio's A w instead of one wave for every 64 rows
        std::vector<int> lr;
        for (int r = 0; r < m; r++)
            if (rptr[r + 1] - rptr[r] > CSR_LONG) lr.push_back(r);
        E.nlr = (int)lr.size();
        E.lrow.ensure(std::max<size_t>(lr.size(), 1));
        if (!lr.empty())
            HIPCHK(hipMemcpyAsync(E.lrow.p, lr.data(), lr.size() * sizeof(int), hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (E.dense) {   // the dense copy is the only one the passes read
        E.cind.release(); E.cval.release();
        E.cind.ensure(1); E.cval.ensure(1);
    }
    E.a_version = lp->a_version;
}

// set_aux_bnds (glpspx02.js:1317-1359) on the device, into separate arrays:
// the auxiliary bounds of every variable from its original type, and the
// status of every non-basic position from the sign of its reduced cost
__global__ void k_aux_bnds(int m, int n, const signed char *__restrict__ orig_type, const int *__restrict__ head,
                           const double *__restrict__ cbar, double *__restrict__ lb, double *__restrict__ ub,
                           signed char *__restrict__ stat, const DState *st, int need_p)
{
    GATE(st, need_p);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;       // variable k + 1
    if (k < m + n) {
        const int t = orig_type[k];
        lb[k] = t == FR ? -1e3 : (t == LO ? 0.0 : (t == UP ? -1.0 : 0.0));
        ub[k] = t == FR ? +1e3 : (t == LO ? +1.0 : (t == UP ? 0.0 : 0.0));
    }
    if (k < n) {
        const int v = head[m + k] - 1;
        const int t = orig_type[v];
        stat[k] = (t != FR && t != LO && t != UP) ? NS : (cbar[k] >= 0.0 ? NL : NU);
    }
}

// set_aux_bnds (glpspx02.js:1317-1359, aux = 1) or set_orig_bnds (:1361-1408,
// aux = 0) on the device, from its own copy of the original types and
// bounds and its reduced costs: the types and bounds of every variable and
// the status of every non-basic position (the host repeats the same rules on
// its mirrors: Spx::set_aux_bnds / set_orig_bnds).  Gated for the end-of-call
// epilogue (epi_arm).
__global__ void k_bounds(int m, int n, int aux, const signed char *__restrict__ orig_type,
                         const double *__restrict__ orig_lb, const double *__restrict__ orig_ub,
                         const int *__restrict__ head, const double *__restrict__ cbar, signed char *__restrict__ type,
                         double *__restrict__ lb, double *__restrict__ ub, signed char *__restrict__ stat,
                         const DState *st, int need_p)
{
    GATE(st, need_p);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m + n) {
        const int t = orig_type[k];
        if (!aux) {
            type[k] = (signed char)t;
            lb[k] = orig_lb[k];
            ub[k] = orig_ub[k];
        } else {
            switch (t) {
            case FR: type[k] = DB; lb[k] = -1e3; ub[k] = +1e3; break;
            case LO: type[k] = DB; lb[k] = 0.0; ub[k] = +1.0; break;
            case UP: type[k] = DB; lb[k] = -1.0; ub[k] = 0.0; break;
            default: type[k] = FX; lb[k] = 0.0; ub[k] = 0.0; break;
            }
        }
    }
    if (k < n) {
        const int v = head[m + k] - 1;
        const int t = orig_type[v];
        const double d = cbar[k];
        signed char sv;
        if (aux) {
            sv = (t != FR && t != LO && t != UP) ? NS : (d >= 0.0 ? NL : NU);
        } else {
            switch (t) {
            case FR: sv = NF; break;
            case LO: sv = NL; break;
            case UP: sv = NU; break;
            case DB:
                if (d >= +DBL_EPSILON) sv = NL;
                else if (d <= -DBL_EPSILON) sv = NU;
                else sv = (fabs(orig_lb[v]) <= fabs(orig_ub[v])) ? NL : NU;
                break;
            default: sv = NS; break;
            }
        }
        stat[k] = sv;
    }
}

// the state into its slot in front of the pull region (the epilogue's one
// download covers both); not gated: the host reads the state either way
__global__ void k_st_copy(const DState *__restrict__ st, DState *__restrict__ dst)
{
    const unsigned *a = (const unsigned *)st;
    unsigned *b = (unsigned *)dst;
    for (int i = threadIdx.x; i < (int)(sizeof(DState) / 4); i += blockDim.x) b[i] = a[i];
}

// The phase-I epilogue's step between eval_cbar and eval_beta, one thread
// per variable k: check_stab (glpspx02.js:1410) and check_feas (:1296) of the
// fresh reduced cost at k's non-basic position against the status the batch
// left (block b's two flags to flags[2 b], flags[2 b + 1], ORed by the host),
// set_orig_bnds (:1361) for k (k_bounds' rules: type, bounds, status), and
// eval_beta's right-hand side split (k_split_pos mode 0: ys / wc from the new
// status and bounds) — three launches' work in one
__global__ void __launch_bounds__(256) k_epi_orig(int m, int n, const signed char *__restrict__ orig_type,
                                                  const double *__restrict__ orig_lb, const double *__restrict__ orig_ub,
                                                  const int *__restrict__ bind, const double *__restrict__ cbar,
                                                  signed char *__restrict__ type, double *__restrict__ lb,
                                                  double *__restrict__ ub, signed char *__restrict__ stat,
                                                  double *__restrict__ ys, double *__restrict__ wc, double tol_dj,
                                                  int *flags, const DState *st, int need_p)
{
    GATE(st, need_p);
    __shared__ int red[2][4];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;      // variable k + 1
    int stab = 0, inf = 0;
    if (k < m + n) {
        const int t = orig_type[k];
        const double l = orig_lb[k], u = orig_ub[k];
        type[k] = (signed char)t;
        lb[k] = l;
        ub[k] = u;
        const int pos = bind[k];
        double v = 0.0;
        if (pos > m) {
            const int j = pos - m - 1;
            const double d = cbar[j];
            const int s0 = stat[j];
            if (d < -tol_dj) {
                stab = (s0 == NL || s0 == NF);
                inf = (t == LO || t == FR);
            }
            if (d > +tol_dj) {
                stab |= (s0 == NU || s0 == NF);
                inf |= (t == UP || t == FR);
            }
            int sv;
            switch (t) {
            case FR: sv = NF; break;
            case LO: sv = NL; break;
            case UP: sv = NU; break;
            case DB:
                if (d >= +DBL_EPSILON) sv = NL;
                else if (d <= -DBL_EPSILON) sv = NU;
                else sv = (fabs(l) <= fabs(u)) ? NL : NU;
                break;
            default: sv = NS; break;
            }
            stat[j] = (signed char)sv;
            v = -(sv == NU ? u : (sv == NF ? 0.0 : l));         // -get_xN
        }
        if (k < m) ys[k] = v;
        else wc[k - m] = v;
    }
    stab = __any(stab);
    inf = __any(inf);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][w] = stab;
        red[1][w] = inf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        flags[2 * blockIdx.x] = red[0][0] | red[0][1] | red[0][2] | red[0][3];
        flags[2 * blockIdx.x + 1] = red[1][0] | red[1][1] | red[1][2] | red[1][3];
    }
}

static double bits_double(unsigned long long b)
{
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// GK_DET_LOG=<file> (tools/det_probe.py): a fingerprint of the device state
// after every batch and re-inversion — a wrapping sum of mixed (index, word)
// pairs, independent of the summation order — so that two solves of the same
// input can be compared batch by batch and the first divergence located
__global__ void k_det_hash(const unsigned *__restrict__ w, size_t nw, unsigned long long *out)
{
    unsigned long long acc = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)w[i] << 17 | w[i]);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        acc += z ^ (z >> 31);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

static const char *det_log_path()
{
    static const char *p = std::getenv("GK_DET_LOG");
    return p;
}

// ---------------------------------------------------------------------------
// the simplex driver
// ---------------------------------------------------------------------------
struct Spx {
    gk_ctx *ctx;
    gk_bfd *f;
    Engine *E;
    gk_lp *lp;
    const gk_smcp *parm;
    int m, n, dual;
    hipStream_t s;
    // host mirrors (1-based like the reference csa)
    std::vector<signed char> type, orig_type, stat;
    std::vector<double> lb, ub, coef, orig_lb, orig_ub, obj, bbar, cbar, gamma;
    std::vector<int> head, bind;
    double zeta = 0.0, tm_beg = 0.0;
    int phase = 0, it_beg = 0;
    DState hs{};
    bool dinf_known = false;
    bool head_stale = false, vec_stale = false;
    // the device's cbar / bbar equal a fresh eval_cbar / eval_bbar of the
    // current device state (basis, costs, bounds, factor and list order):
    // the evaluation is deterministic, so repeating it is skipped.  Cleared
    // by pivots, re-inversion, list rebuilds, and cost / bound changes.
    bool cbar_ok = false, bbar_ok = false;
    int evals_skipped = 0;
    // the end-of-call epilogue (epi_arm): the evaluations the host takes up
    // after the batch that reaches the iteration limit, enqueued behind that
    // batch and gated on its budget, with their results downloaded in the
    // same wait.  eg / eg_nr: the gate and the bound of the list length that
    // the eval routines' launches take while it is enqueued
    const DState *eg = nullptr;
    int eg_nr = 0;
    struct Epi {
        bool ready = false;                // the batch ran to its budget: the results below are current
        bool has_cbar = false, has_bbar = false;
        bool bounds_pending = false;       // phase I: set_orig_bnds ran on the device (bbar is under them)
        bool aux = false;                  // next_aux's evaluation launched too
        bool checks = false;               // phase I: check_stab / check_feas evaluated on the device
        int stab = 0, feas = 0;
        std::vector<signed char> stat;     // the statuses the epilogue's set_orig_bnds gave
    } epi;
    void epi_drop() { epi.ready = epi.has_cbar = epi.has_bbar = epi.bounds_pending = epi.aux = epi.checks = false; }

    SpxDev dev() const
    {
        SpxDev d;
        std::memset(&d, 0, sizeof(d));      // compared bytewise by the graph cache
        d.m = m; d.n = n; d.A = E->mat();
        d.type = E->type.p; d.orig_type = E->orig_type.p; d.stat = E->stat.p; d.refsp = E->refsp.p;
        d.lb = E->lb.p; d.ub = E->ub.p; d.coef = E->coef.p; d.orig_lb = E->orig_lb.p; d.orig_ub = E->orig_ub.p;
        d.obj = E->obj.p; d.head = E->head.p; d.bind = E->bind.p;
        d.bbar = E->bbar.p; d.cbar = E->cbar.p; d.gamma = E->gamma.p;
        d.tcol = E->tcol.p; d.trow = E->trow.p; d.rho = E->rho.p; d.rowp = E->rowp.p; d.u = E->u.p; d.s = E->s.p;
        d.h = E->h.p; d.wcol = E->wcol.p; d.ys = E->ys.p; d.work = E->work.p; d.r1 = E->r1.p; d.r2 = E->r2.p;
        d.Binv = f->Binv.p; d.ldb = f->ldb;
        d.partial = E->partial.p; d.partial_cap = PARTIAL_CAP;
        d.st = E->st.p;
        d.rlist = E->rlist.p; d.rpos = E->rpos.p; d.rho_idx = E->rho_idx.p; d.rho_val = E->rho_val.p;
        d.gpart = E->gpart.p;
        d.wlist = E->wlist.p; d.wpos = E->wpos.p; d.cand = E->cand.p;
        d.awpart = E->awpart.p; d.awpart_cap = (size_t)AW_SPLITS * m; d.awcnt = E->awcnt.p;
        if (E->pnl_m == m && E->pnl_n == n) {
            d.pnl = E->pnl.p; d.pnl_src = E->pnl_src.p; d.pslot = E->pslot.p; d.ppos = E->ppos.p;
            d.ldp = (n + 7) & ~7;
        }
        // the roofline stamps (per-block exit clocks, kernel spans, algorithmic
        // bytes) cost stores and a reduction on the critical path of every
        // pivot: they run only while a profiling mode is on (gk_bfd_profile)
        d.sp = f->sparse ? f->sp : nullptr;
        d.shard = (f->shard && E->dense && !f->sparse && dual) ? f->shard : nullptr;
        d.tslots = E->prof ? E->tslots.p : nullptr;
        d.xslots = E->prof ? E->xslots.p : nullptr;
        d.trace = nullptr;
        if (E->prof == 2 || E->prof == 3) {
            if (!E->trace.p) {
                E->trace.ensure(TRACE_LEN);
                HIPCHK(hipMemset(E->trace.p, 0, E->trace.n * sizeof(unsigned long long)));
            }
            d.trace = E->trace.p;
        }
        return d;
    }

    template <typename T>
    void up(DBuf<T> &d, const std::vector<T> &h, size_t cnt)
    {
        // through the pinned staging buffer: the host data is taken now, the
        // copy itself is asynchronous (or, between begin_up and flush_up, one
        // copy of the whole staged region plus a device-side scatter)
        const size_t bytes = cnt * sizeof(T);
        char *stage = pin_take(bytes);
        if (!stage) {
            HIPCHK(hipMemcpyAsync(d.p, h.data() + 1, bytes, hipMemcpyHostToDevice, s));
            return;
        }
        std::memcpy(stage, h.data() + 1, bytes);
        if (coalesce) {
            segs.push_back(UpSeg{(size_t)(stage - E->pin) - coal_beg, (void *)d.p, bytes});
            return;
        }
        HIPCHK(hipMemcpyAsync(d.p, stage, bytes, hipMemcpyHostToDevice, s));
    }
    bool coalesce = false;
    size_t coal_beg = 0;
    std::vector<UpSeg> segs;
    void begin_up()
    {
        // start from an empty staging buffer (it holds 32 (m + n + 1)
        // doubles, more than init's uploads: no sync inside the region)
        if (pin_off) sync();
        coalesce = true;
        coal_beg = pin_off;
        segs.clear();
    }
    void flush_up()
    {
        coalesce = false;
        if (segs.empty()) return;
        // the segment table behind the data, then one copy and one kernel
        char *tab = pin_take(segs.size() * sizeof(UpSeg));
        if (!tab) {
            for (const UpSeg &g : segs)
                HIPCHK(hipMemcpyAsync(g.dst, E->pin + coal_beg + g.off, g.bytes, hipMemcpyHostToDevice, s));
            segs.clear();
            return;
        }
        std::memcpy(tab, segs.data(), segs.size() * sizeof(UpSeg));
        const size_t total = pin_off - coal_beg;
        ctx->upstage.ensure(E->pin_cap);
        E->upstage.view(ctx->upstage.p, ctx->upstage.n);
        HIPCHK(hipMemcpyAsync(E->upstage.p, E->pin + coal_beg, total, hipMemcpyHostToDevice, s));
        scatter_segments(s, E->upstage.p, (const UpSeg *)(E->upstage.p + (tab - (E->pin + coal_beg))),
                         (int)segs.size());
        segs.clear();
    }
    template <typename T>
    void down(std::vector<T> &h, const DBuf<T> &d, size_t cnt)
    {
        // into the pinned staging buffer; the host vector is filled by the
        // sync() that every download is followed by
        const size_t bytes = cnt * sizeof(T);
        char *stage = pin_take(bytes);
        if (!stage) {
            HIPCHK(hipMemcpyAsync(h.data() + 1, d.p, bytes, hipMemcpyDeviceToHost, s));
            return;
        }
        HIPCHK(hipMemcpyAsync(stage, d.p, bytes, hipMemcpyDeviceToHost, s));
        pending.push_back(Pending{(void *)(h.data() + 1), stage, bytes});
    }
    struct Pending {
        void *dst;
        const char *src;
        size_t bytes;
    };
    std::vector<Pending> pending;
    size_t pin_off = 0;
    char *pin_take(size_t bytes)
    {
        const size_t need = (bytes + 255) & ~(size_t)255;
        if (need > E->pin_cap) return nullptr;
        if (pin_off + need > E->pin_cap) sync();
        char *p = E->pin + pin_off;
        pin_off += need;
        return p;
    }
    void sync()
    {
        HIPCHK(hipStreamSynchronize(s));
        f->stats.host_syncs++;
        for (const Pending &q : pending) std::memcpy(q.dst, q.src, q.bytes);
        pending.clear();
        pin_off = 0;
    }

    // GK_CALL_LOG: the host timeline of one call (label, seconds), printed
    // at its end — where the host time between the device's work goes
    std::vector<std::pair<const char *, double>> marks;
    void mark(const char *what)
    {
        static const bool on = std::getenv("GK_CALL_LOG") != nullptr;
        if (on) marks.emplace_back(what, now_s());
    }
    // bring the host mirrors of the pivot-updated arrays up to date
    void pull()
    {
        if (!head_stale && !vec_stale) return;
        mark("pull");
        pull_enqueue();
        sync();
        head_stale = vec_stale = false;
        mark("pull done");
    }
    void pull_enqueue()
    {
        // head | bind | stat | bbar | cbar (| coef) lie contiguous in the
        // arena (engine_alloc): one copy into the pinned staging buffer
        const char *lo = (const char *)E->head.p;
        const char *hi = dual ? (const char *)(E->cbar.p + n) : (const char *)(E->coef.p + m + n);
        char *stage = pin_take((size_t)(hi - lo));
        if (!stage) {
            down(head, E->head, (size_t)m + n);
            down(bind, E->bind, (size_t)m + n);
            down(stat, E->stat, n);
            down(bbar, E->bbar, m);
            down(cbar, E->cbar, n);
            if (!dual) down(coef, E->coef, (size_t)m + n);
        } else {
            HIPCHK(hipMemcpyAsync(stage, lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, s));
            auto take = [&](void *dst, const void *src, size_t bytes) {
                pending.push_back(Pending{dst, stage + ((const char *)src - lo), bytes});
            };
            take(head.data() + 1, E->head.p, ((size_t)m + n) * sizeof(int));
            take(bind.data() + 1, E->bind.p, ((size_t)m + n) * sizeof(int));
            take(stat.data() + 1, E->stat.p, (size_t)n);
            take(bbar.data() + 1, E->bbar.p, (size_t)m * sizeof(double));
            take(cbar.data() + 1, E->cbar.p, (size_t)n * sizeof(double));
            if (!dual) take(coef.data() + 1, E->coef.p, ((size_t)m + n) * sizeof(double));
        }
    }
    void push_state()
    {
        // through its own slot of the staging ring: the copy may still be
        // queued when the host writes the next state (init returns without
        // waiting for its uploads)
        char *stage = pin_take(sizeof(DState));
        if (!stage) {
            *E->st_host = hs;
            HIPCHK(hipMemcpyAsync(E->st.p, E->st_host, sizeof(DState), hipMemcpyHostToDevice, s));
            sync();
            return;
        }
        std::memcpy(stage, &hs, sizeof(DState));
        HIPCHK(hipMemcpyAsync(E->st.p, stage, sizeof(DState), hipMemcpyHostToDevice, s));
    }
    void pull_state()
    {
        HIPCHK(hipMemcpyAsync(E->st_host, E->st.p, sizeof(DState), hipMemcpyDeviceToHost, s));
        sync();
        hs = *E->st_host;
    }

    double get_xN(int j) const
    {
        int k = head[m + j];
        switch (stat[j]) {
        case NL: return lb[k];
        case NU: return ub[k];
        case NF: return 0.0;
        default: return lb[k];
        }
    }

    // ---- device computations between batches ------------------------------
    // y = inv(B) x / inv(B)' x: over the dense columns only in the dual path
    // (rlist maintained by the pivot kernels), all m columns otherwise
    static constexpr int LIST_FTRAN_MAX = 2048;
    // rlist is exact in the dual always, in the primal unless a batch of the
    // single-workgroup (rigorous) kernels ran since the last rebuild
    bool lists_ok() const { return dual || !lists_stale; }
    void ftran_(const double *x, double *y)
    {
        if (eg) { binv_ftran_list(s, dev(), eg_nr, x, y, eg); return; }      // (epi_arm: the list form holds)
        if (f->sparse) { sp_ftran(*f->sp, s, x, y); return; }
        if (lists_ok() && hs.nr <= LIST_FTRAN_MAX) binv_ftran_list(s, dev(), hs.nr, x, y);
        else gemv_n(s, f->Binv.p, m, m, f->ldb, x, E->partial.p, PARTIAL_CAP, y, 1.0, nullptr, 0.0);
    }
    void btran_(const double *x, double *y)
    {
        if (eg) { binv_btran_list(s, dev(), eg_nr, x, y, eg); return; }
        if (f->sparse) { sp_btran(*f->sp, s, x, y); return; }
        if (lists_ok()) binv_btran_list(s, dev(), hs.nr, x, y);
        else gemv_t(s, f->Binv.p, m, m, f->ldb, x, y, 1.0);
    }
    // eval_cbar (glpspx01.js:565): pi = inv(B') cB refined once, d_j = c_k - N_j' pi
    void eval_cbar()
    {
        if (cbar_ok) { evals_skipped++; return; }
        if (epi.ready && epi.has_cbar) {
            // the epilogue behind the last batch evaluated it (epi_arm; the
            // mirror holds it)
            epi.has_cbar = false;
            cbar_ok = true;
            evals_skipped++;
            return;
        }
        mark("eval_cbar");
        const double t0 = now_s();
        struct T { gk_bfd *f; double t0; ~T() { f->stats.seconds_eval += now_s() - t0; } } tt{f, t0};
        eval_cbar_dev();
        down(cbar, E->cbar, n);
        sync();
        cbar_ok = true;
        mark("eval_cbar done");
    }
    // the device part of eval_cbar: E->cbar
    void eval_cbar_dev()
    {
        SpxDev d = dev();
        MatDev A = E->mat();
        double *cB = E->r1.p, *pi = E->u.p, *r = E->r2.p, *dd = E->work.p;
        cb_vector(s, m, E->head.p, E->coef.p, cB, eg, eg ? EPI_GATE : 0);
        btran_(cB, pi);
        // dense A: pi = inv(B)' cB lives on the dense columns of inv(B) and
        // the basic slacks with a nonzero cost (the primal's phase-I costs;
        // none in the dual), so the passes run over those rows of AT
        std::vector<int> extra;
        if (!dual && E->dense && A.AT && lists_ok()) {
            pull();
            for (int i = 1; i <= m; i++)
                if (head[i] <= m && coef[head[i]] != 0.0) extra.push_back(head[i] - 1);
        }
        const int nrb = eg ? eg_nr : hs.nr;    // (epi_arm: a bound of the finished batch's nr)
        const bool rows = E->dense && A.AT && lists_ok() && nrb <= LIST_FTRAN_MAX && 2 * (nrb + (int)extra.size()) <= m;
        ABI_REQUIRE(!eg || (rows && extra.empty()), "spx: epilogue eval_cbar off the list form");
        if (rows && !extra.empty()) {
            E->xlist.ensure(extra.size());
            HIPCHK(hipMemcpyAsync(E->xlist.p, extra.data(), extra.size() * sizeof(int), hipMemcpyHostToDevice, s));
            sync();
        }
        const int nx = rows ? (int)extra.size() : 0;
        if (rows) rowpass_pi(s, d, CP_RESID, nrb, pi, cB, r, E->xlist.p, nx, eg);
        else colpass(s, A, CP_RESID, 0, m, E->head.p, E->stat.p, E->coef.p, cB, pi, nullptr, r, nullptr, nullptr);
        btran_(r, dd);
        if (rows) {
            // pi += dd (the refinement) inside the pass
            rowpass_pi(s, d, CP_CBAR, nrb, pi, nullptr, E->cbar.p, E->xlist.p, nx, eg, dd);
        } else {
            vec_axpy(s, pi, dd, 1.0, m, eg, eg ? EPI_GATE : 0);
            colpass(s, A, CP_CBAR, m, n, E->head.p, E->stat.p, E->coef.p, nullptr, pi, nullptr, E->cbar.p, nullptr, nullptr);
        }
    }

    // eval_beta (glpspx01.js:473): h = -N xN; beta = inv(B) h, refined once
    // (refine_ftran :251: beta += inv(B) (h - B beta))
    void eval_bbar()
    {
        if (bbar_ok) { evals_skipped++; return; }
        if (epi.ready && epi.has_bbar && !epi.bounds_pending) {
            epi.has_bbar = false;
            bbar_ok = true;
            evals_skipped++;
            return;
        }
        mark("eval_bbar");
        const double t0 = now_s();
        struct T { gk_bfd *f; double t0; ~T() { f->stats.seconds_eval += now_s() - t0; } } tt{f, t0};
        if (next_aux_take()) {
            // evaluated at the end of the last call with exactly these bounds,
            // statuses, basis and factor (the same kernels, so the same bits);
            // the host mirror follows with the next pull (phase I reads it
            // only after the first batch)
            HIPCHK(hipMemcpyAsync(E->bbar.p, E->bbar_n.p, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s));
            evals_skipped++;
            vec_stale = true;
            bbar_ok = true;
            mark("eval_bbar done");
            return;
        }
        eval_bbar_into(dev(), E->bbar.p);
        down(bbar, E->bbar, m);
        sync();
        bbar_ok = true;
        mark("eval_bbar done");
    }
    // h = -N xN over the statuses and bounds of d; beta = inv(B) h, refined once
    // (split_done: ys / wc of the right-hand side are in place — k_epi_orig)
    void eval_bbar_into(const SpxDev &d, double *beta, bool split_done = false)
    {
        MatDev A = E->mat();
        double *ys = E->r1.p, *wc = E->wcol.p, *h = E->h.p, *t = E->r2.p, *dd = E->work.p;
        const int gm = eg ? EPI_GATE : 0;
        if (!split_done) split_pos(s, d, 0, nullptr, ys, wc, eg, gm);
        aprod_neg_gated(s, A, wc, ys, h, E->partial.p, PARTIAL_CAP, eg, gm);    // h = ys - A wc
        ftran_(h, beta);
        split_pos(s, d, 1, beta, ys, wc, eg, gm);
        if (A.dense) {
            // t = h - B beta in the product's reduction pass
            aprod_neg_gated(s, A, wc, ys, t, E->partial.p, PARTIAL_CAP, eg, gm, h);
        } else {
            aprod_neg_gated(s, A, wc, ys, t, E->partial.p, PARTIAL_CAP, eg, gm);  // t = B beta
            rsub_into(t, h);                                                       // t = h - B beta
        }
        if (eg || (!f->sparse && lists_ok() && hs.nr <= LIST_FTRAN_MAX)) {
            // beta += inv(B) t in the list FTRAN's pass (ftran_'s list form)
            binv_ftran_list(s, dev(), eg ? eg_nr : hs.nr, t, beta, eg, 1);
        } else {
            ftran_(t, dd);
            vec_axpy(s, beta, dd, 1.0, m, eg, gm);
        }
    }
    // A dual call that stops on its iteration / time limit in phase I leaves
    // its basis for the next call, which (the reference's spx_dual from the
    // top: init_csa, eval_cbar, check_feas, set_aux_bnds) evaluates the basic
    // values under the auxiliary bounds again.  The reduced costs that call
    // derives the statuses from are the ones this call just evaluated, so the
    // evaluation can run now, on the device, while the host returns and the
    // caller prepares the next call — the same kernels on the same inputs,
    // bit for bit the result that call would compute.  next_aux_take uses it
    // only when everything it depends on is unchanged: the resident working
    // set was kept (same matrix, bounds, costs, basis, factor), no pivot and
    // no re-inversion happened yet in this call, and set_aux_bnds gave every
    // non-basic variable the status the evaluation used.
    void next_aux_launch()
    {
        Engine::NextAux &X = E->next_aux;
        X.ok = false;
        const char *ev = std::getenv("GK_NEXT_AUX");         // 0: off (A/B tests)
        if (ev && std::atoi(ev) == 0) return;
        if (!dual || phase != 1 || head_stale || vec_stale) return;
        const size_t mn = (size_t)m + n;
        if (epi.ready && epi.aux)
            epi.aux = false;           // the epilogue launched it from the same cbar and header (epi_arm)
        else
            next_aux_dev();
        // the host record: the same rule on the host mirrors (cbar is the
        // fresh evaluation the device holds)
        X.stat_var.assign(mn + 1, 0);
        for (int j = 1; j <= n; j++) {
            const int k = head[m + j];
            const int t = orig_type[k];
            X.stat_var[k] = (t != FR && t != LO && t != UP) ? NS : (cbar[j] >= 0.0 ? NL : NU);
        }
        X.fact_ver = f->fact_ver;
        X.ok = true;
    }
    void next_aux_dev()
    {
        const size_t mn = (size_t)m + n;
        E->lb_n.ensure(mn); E->ub_n.ensure(mn); E->stat_n.ensure(n); E->bbar_n.ensure(m);
        hipLaunchKernelGGL(k_aux_bnds, dim3((unsigned)((std::max<size_t>(mn, n) + 255) / 256)), dim3(256), 0, s, m, n,
                           E->orig_type.p, E->head.p, E->cbar.p, E->lb_n.p, E->ub_n.p, E->stat_n.p, eg,
                           eg ? EPI_GATE : 0);
        SpxDev d = dev();
        d.lb = E->lb_n.p; d.ub = E->ub_n.p; d.stat = E->stat_n.p;
        eval_bbar_into(d, E->bbar_n.p);
    }
    bool next_aux_take()
    {
        Engine::NextAux &X = E->next_aux;
        if (!X.ok) return false;
        X.ok = false;                                  // one use
        if (!dual || phase != 1 || !kept || reinv_calls || hs.it_cnt != it_beg || f->fact_ver != X.fact_ver ||
            X.stat_var.size() != (size_t)m + n + 1)
            return false;
        for (int j = 1; j <= n; j++)
            if (stat[j] != X.stat_var[head[m + j]]) return false;
        return true;
    }
    bool kept = false;                                 // init kept the resident working set
    int reinv_calls = 0;                               // re-inversions in this call

    // one GK_DET_LOG line: the state fingerprints after a batch / re-inversion
    void det_log(const char *what, int K = 0, int why = 0)
    {
        const char *path = det_log_path();
        if (!path) return;
        const size_t ldb = f->sparse ? 0 : (size_t)f->ldb;
        struct Part { const void *p; size_t bytes; } parts[6] = {
            {E->head.p, ((size_t)m + n) * sizeof(int)}, {E->stat.p, (size_t)n & ~(size_t)3},
            {E->bbar.p, (size_t)m * sizeof(double)}, {E->cbar.p, (size_t)n * sizeof(double)},
            {E->gamma.p, (size_t)(dual ? m : n) * sizeof(double)}, {f->Binv.p, ldb * m * sizeof(double)}};
        E->dethash.ensure(6);
        HIPCHK(hipMemsetAsync(E->dethash.p, 0, 6 * sizeof(unsigned long long), s));
        for (int t = 0; t < 6; t++)
            if (parts[t].p && parts[t].bytes >= 4)
                hipLaunchKernelGGL(k_det_hash, dim3(512), dim3(256), 0, s, (const unsigned *)parts[t].p,
                                   parts[t].bytes / 4, E->dethash.p + t);
        unsigned long long hsh[6];
        HIPCHK(hipMemcpyAsync(hsh, E->dethash.p, sizeof hsh, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        FILE *fp = std::fopen(path, "a");
        if (!fp) return;
        std::fprintf(fp, "%s it %d K %d why %d p %d q %d ph %d nr %d upd %d/%d head %016llx stat %016llx bbar %016llx "
                     "cbar %016llx gamma %016llx binv %016llx\n", what, hs.it_cnt, K, why, hs.p, hs.q, phase, hs.nr,
                     hs.upd_cnt, hs.upd_lim, hsh[0], hsh[1], hsh[2], hsh[3], hsh[4], hsh[5]);
        std::fclose(fp);
    }

    void rsub_into(double *y, const double *a);   // y = a - y

    bool reinvert()
    {
        epi_drop();
        pull();
        reinv_calls++;
        cbar_ok = bbar_ok = false;
        hs.pvalid = 0;                          // the pricing panel is refilled from the fresh inverse
        BasisSplit bs;
        if (!split_from_head(m, head.data(), bs)) {
            fact_ret = 1;                       // BFD_ESING
            return false;
        }
        MatDev A = E->mat();
        int ret;
        const bool refine = refine_next;
        refine_next = false;
        echk_seen = hs.echk;
        if (f->sparse) {
            ret = sparse_reinvert();
            fact_ret = ret;
            return ret == 0;
        }
        if (E->dense)
            ret = reinvert_core(f, bs, &A, 0, 1.0, nullptr, nullptr, nullptr, refine);
        else
            ret = reinvert_core_csc(bs, refine);
        fact_ret = ret;
        return ret == 0;
    }
    int fact_ret = 0;
    int sp_replayed = 0;                     // pivots the look-ahead's factor was given back (the chain's length)
    // B0 = L U of the current basis on the host (gk_sparse.hip), uploaded;
    // or, at a scheduled refactorization, the look-ahead's factor of an
    // earlier basis of the chain with the later pivots replayed onto it
    int sparse_reinvert()
    {
        const double t0 = now_s();
        int ret;
        sp_replayed = 0;
        if (sp_ahead_mark(*f->sp) >= 0) {
            if (f->valid && hs.upd_cnt >= hs.upd_lim) {
                MatDev A = E->mat();
                double tw = 0.0;
                const int r = sp_ahead_install(*f->sp, s, -1, A.cptr, A.cind, A.cval, E->h.p, &tw);
                if (r >= 0) {
                    sp_replayed = r;
                    f->fact_ver++;
                    f->valid = 1;
                    f->upd_cnt = r;
                    f->ext_upd = 0;
                    f->stats.reinversions++;
                    f->stats.lu_ahead++;
                    f->stats.seconds_lu += tw;             // the LU time the pivots did not hide
                    f->stats.seconds_reinvert += now_s() - t0;
                    static const bool slog = std::getenv("GK_SPARSE_LOG") != nullptr;
                    if (slog)
                        fprintf(stderr, "[gk sparse] it %d: look-ahead factor, %d pivots replayed, join waited %.2f ms, "
                                "refactor %.2f ms\n", hs.it_cnt, r, 1e3 * tw, 1e3 * (now_s() - t0));
                    return 0;
                }
            } else
                sp_ahead_cancel(*f->sp);
        }
        try {
            ret = sp_factorize(*f->sp, s, m, head.data(), E->hcptr.data(), E->hcind.data(), E->hcval.data(),
                               f->parm.piv_tol, f->parm.piv_lim, f->parm.eps_tol);
        } catch (const std::exception &e) {
            throw AbiError{e.what()};
        }
        f->fact_ver++;
        f->valid = ret == 0;
        f->upd_cnt = 0;
        f->ext_upd = 0;
        f->stats.reinversions++;
        f->stats.seconds_reinvert += now_s() - t0;
        {
            long long nnz_lu = 0;
            int lv[4];
            double tl = 0.0;
            sp_info(f->sp, &nnz_lu, lv, &tl);
            f->stats.seconds_lu += tl;
        }
        static const bool slog = std::getenv("GK_SPARSE_LOG") != nullptr;
        if (slog && ret == 0) {
            long long nnz = 0;
            int lev[4];
            double tlu = 0.0;
            sp_info(f->sp, &nnz, lev, &tlu);
            fprintf(stderr, "[gk sparse] it %d: nnz(L+U) %lld, levels FTRAN %d + %d, BTRAN %d + %d, host LU %.2f ms, "
                    "refactor %.2f ms\n", hs.it_cnt, nnz, lev[0], lev[1], lev[2], lev[3], 1e3 * tlu,
                    1e3 * (now_s() - t0));
        }
        return ret ? 1 : 0;
    }
    // the next re-inversion is a scheduled one (update limit, no growth-check
    // failure since the last): inv(B) is the updated inverse of the current
    // basis and may be refined instead of rebuilt (gk_newton.hip)
    bool refine_next = false;
    int echk_seen = 0;

    // the sparse factor's look-ahead (GK_SP_AHEAD: the pivots before the
    // update limit at which the next LU starts on a host thread; 0 turns it
    // off): the basis at that point of the chain is factorized while the
    // device pivots on, and the pivots since are replayed at the
    // refactorization (sp_ahead_install).  The start is a pivot count, not a
    // time, so the path stays deterministic; the default covers a host LU of
    // ~40 ms (m = 100k) at ~1,000 pivots/s and costs ~32 replayed FTRANs
    static int ahead_lead()
    {
        static const int lead = [] {
            const char *e = std::getenv("GK_SP_AHEAD");
            return e ? std::atoi(e) : 32;
        }();
        return lead;
    }
    static int ahead_min_m()                 // GK_SP_AHEAD_MIN_M: the smallest m the look-ahead runs at
    {
        static const int v = [] {
            const char *e = std::getenv("GK_SP_AHEAD_MIN_M");
            return e ? std::atoi(e) : 50000;
        }();
        return v;
    }
    // a batch that would run past the look-ahead's starting point ends
    // there, so that the host LU gets the whole lead (batches of up to 64
    // pivots otherwise started it as few as 8 pivots before the limit)
    int ahead_align(int K) const
    {
        const int lead = ahead_lead();
        if (!f->sparse || lead <= 0 || m < ahead_min_m() || !f->valid || sp_ahead_mark(*f->sp) >= 0 ||
            hs.upd_lim < 2 * lead)
            return K;
        const int left = hs.upd_lim - lead - hs.upd_cnt;
        return (left > 0 && left < K) ? left : K;
    }
    void ahead_maybe()
    {
        const int lead = ahead_lead();
        // (below m = 50,000 the host LU takes a few ms: replaying the lead's
        // FTRANs would cost more than it hides)
        if (lead <= 0 || m < ahead_min_m() || !f->valid || sp_ahead_mark(*f->sp) >= 0 || hs.npiv == 0 ||
            hs.refact_pending)
            return;
        if (hs.upd_lim < 2 * lead || hs.upd_cnt >= hs.upd_lim || hs.upd_cnt < hs.upd_lim - lead) return;
        pull();
        sp_ahead_start(*f->sp, m, head.data(), E->hcptr.data(), E->hcind.data(), E->hcval.data(), f->parm.piv_tol,
                       f->parm.piv_lim, f->parm.eps_tol, sp_log_count(*f->sp, s));
    }

    // ---- the reference's terminal output (display, glpspx01.js:1550-1589 /
    // glpspx02.js:1452-1497, and the xprintf lines of the main loops), as
    // structured reports: the host formats them with its own number
    // printing (the reference prints doubles with JavaScript's conversion)
    int it_dpy = -1;
    void report_msg(int code, int lev, int aux = 0)
    {
        if (f->rpt && parm->msg_lev >= lev) f->rpt(f->rpt_ud, GK_RPT_MSG, code, hs.it_cnt, phase, 0.0, 0.0, aux);
    }
    void display(int spec)
    {
        const gk_smcp *P = parm;
        if (!f->rpt || P->msg_lev < 2) return;             // GLP_MSG_ON
        if (P->out_dly > 0 && 1000.0 * (now_s() - tm_beg) < P->out_dly) return;
        if (hs.it_cnt == it_dpy) return;
        if (!spec && hs.it_cnt % std::max(P->out_frq, 1) != 0) return;
        pull();
        double sum = 0.0;
        int cnt = 0;
        if (dual) {
            // the sum of dual infeasibilities (phase I: of the working costs)
            if (phase == 1) {
                for (int i = 1; i <= m; i++) sum -= coef[head[i]] * bbar[i];
                for (int j = 1; j <= n; j++) sum -= coef[head[m + j]] * get_xN(j);
            } else {
                for (int j = 1; j <= n; j++) {
                    if (cbar[j] < 0.0 && (stat[j] == NL || stat[j] == NF)) sum -= cbar[j];
                    if (cbar[j] > 0.0 && (stat[j] == NU || stat[j] == NF)) sum += cbar[j];
                }
            }
            for (int i = 1; i <= m; i++)
                if (orig_type[head[i]] == FX) cnt++;
        } else {
            // the sum of primal infeasibilities of the basic variables
            for (int i = 1; i <= m; i++) {
                const int k = head[i];
                if ((type[k] == LO || type[k] == DB || type[k] == FX) && bbar[i] < lb[k]) sum += lb[k] - bbar[i];
                if ((type[k] == UP || type[k] == DB || type[k] == FX) && bbar[i] > ub[k]) sum += bbar[i] - ub[k];
                if (type[k] == FX) cnt++;
            }
        }
        const double ob = (dual && phase == 1) ? 0.0 : eval_obj();
        f->rpt(f->rpt_ud, GK_RPT_PROGRESS, dual ? 2 : 1, hs.it_cnt, phase, ob, sum, cnt);
        it_dpy = hs.it_cnt;
    }
    // pivots of the next batch: up to the next progress line
    int align_to_display(int K) const
    {
        if (!f->rpt || parm->msg_lev < 2) return K;
        const int fr = std::max(parm->out_frq, 1);
        return std::max(1, std::min(K, fr - hs.it_cnt % fr));
    }
    int reinvert_core_csc(const BasisSplit &bs, bool refine = false);

    // ---- host-side logic on the mirrors -------------------------------------
    // dual: check_feas (glpspx02.js:1296)
    int dual_check_feas(double tol_dj)
    {
        for (int j = 1; j <= n; j++) {
            int k = head[m + j];
            if (cbar[j] < -tol_dj)
                if (orig_type[k] == LO || orig_type[k] == FR) return 1;
            if (cbar[j] > +tol_dj)
                if (orig_type[k] == UP || orig_type[k] == FR) return 1;
        }
        return 0;
    }
    // the host's type / lb / ub hold the auxiliary bounds (the original ones
    // parked in E->auxc) — see set_aux_bnds
    bool cur_aux = false;
    void set_aux_bnds()                                  // glpspx02.js:1317
    {
        // the auxiliary arrays depend on orig_type alone: built once per
        // bounds version into the cache, then swapped with the current
        // (original) arrays, and swapped back by set_orig_bnds
        Engine::AuxCache &C = E->auxc;
        if (!cur_aux) {
            const size_t mn = (size_t)m + n + 1;
            if (!C.ok || C.type.size() != mn) {
                C.type.resize(mn); C.lb.resize(mn); C.ub.resize(mn);
                C.type[0] = 0; C.lb[0] = C.ub[0] = 0.0;
                for (int k = 1; k <= m + n; k++) {
                    switch (orig_type[k]) {
                    case FR: C.type[k] = DB; C.lb[k] = -1e3; C.ub[k] = +1e3; break;
                    case LO: C.type[k] = DB; C.lb[k] = 0.0; C.ub[k] = +1.0; break;
                    case UP: C.type[k] = DB; C.lb[k] = -1.0; C.ub[k] = 0.0; break;
                    default: C.type[k] = FX; C.lb[k] = C.ub[k] = 0.0; break;
                    }
                }
                C.ok = true;
            }
            type.swap(C.type); lb.swap(C.lb); ub.swap(C.ub);
            cur_aux = true;
        }
        for (int j = 1; j <= n; j++) {
            int k = head[m + j];
            if (type[k] == FX) stat[j] = NS;
            else if (cbar[j] >= 0.0) stat[j] = NL;
            else stat[j] = NU;
        }
        push_bounds_dev(1);
    }
    // the original arrays back in the host's type / lb / ub
    void restore_orig_arrays()
    {
        if (cur_aux) {
            Engine::AuxCache &C = E->auxc;
            type.swap(C.type); lb.swap(C.lb); ub.swap(C.ub);
            cur_aux = false;
        } else {
            type = orig_type; lb = orig_lb; ub = orig_ub;
        }
    }
    // push_bounds, with the types, bounds and statuses written by the device
    // from its original arrays and its reduced costs (k_bounds: the device's
    // cbar is the host's here — every caller evaluated it just before)
    void push_bounds_dev(int aux)
    {
        epi_drop();
        bbar_ok = false;
        const int mn = m + n;
        hipLaunchKernelGGL(k_bounds, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, s, m, n, aux, E->orig_type.p,
                           E->orig_lb.p, E->orig_ub.p, E->head.p, E->cbar.p, E->type.p, E->lb.p, E->ub.p, E->stat.p,
                           (const DState *)nullptr, 0);
    }
    void set_orig_bnds()                                 // glpspx02.js:1361
    {
        // (k_bounds ran behind the batch, on the reduced costs the host
        // now holds)
        const bool on_dev = epi.ready && epi.bounds_pending && !epi.has_cbar;
        restore_orig_arrays();
        for (int j = 1; j <= n; j++) {
            int k = head[m + j];
            switch (type[k]) {
            case FR: stat[j] = NF; break;
            case LO: stat[j] = NL; break;
            case UP: stat[j] = NU; break;
            case DB:
                if (cbar[j] >= +DBL_EPSILON) stat[j] = NL;
                else if (cbar[j] <= -DBL_EPSILON) stat[j] = NU;
                else if (std::fabs(lb[k]) <= std::fabs(ub[k])) stat[j] = NL;
                else stat[j] = NU;
                break;
            default: stat[j] = NS; break;
            }
        }
        if (on_dev) {
            ABI_REQUIRE(epi.stat.size() == stat.size() && std::memcmp(epi.stat.data() + 1, stat.data() + 1, n) == 0,
                        "spx: epilogue statuses differ from set_orig_bnds");
            epi.bounds_pending = false;
            bbar_ok = false;
            return;
        }
        push_bounds_dev(0);
    }
    // check_stab and check_feas in one pass over the reduced costs
    int dual_check_stab_feas(double tol_dj, int *feas)
    {
        int stab = 0, inf = 0;
        for (int j = 1; j <= n; j++) {
            const double d = cbar[j];
            const int st = stat[j];
            const int t = orig_type[head[m + j]];
            if (d < -tol_dj) {
                stab |= (st == NL || st == NF);
                inf |= (t == LO || t == FR);
            }
            if (d > +tol_dj) {
                stab |= (st == NU || st == NF);
                inf |= (t == UP || t == FR);
            }
        }
        *feas = inf;
        return stab;
    }
    int dual_check_stab(double tol_dj)                   // glpspx02.js:1410
    {
        for (int j = 1; j <= n; j++) {
            if (cbar[j] < -tol_dj)
                if (stat[j] == NL || stat[j] == NF) return 1;
            if (cbar[j] > +tol_dj)
                if (stat[j] == NU || stat[j] == NF) return 1;
        }
        return 0;
    }
    // primal: set_aux_obj / set_orig_obj / check_stab / check_feas (glpspx01.js:1373-1522)
    int set_aux_obj(double tol_bnd)
    {
        cbar_ok = false;
        int cnt = 0;
        tol_bnd *= 0.90;
        for (int k = 1; k <= m + n; k++) coef[k] = 0.0;
        for (int i = 1; i <= m; i++) {
            int k = head[i];
            if (type[k] == LO || type[k] == DB || type[k] == FX) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(lb[k]));
                if (bbar[i] < lb[k] - eps) { coef[k] = -1.0; cnt++; }
            }
            if (type[k] == UP || type[k] == DB || type[k] == FX) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(ub[k]));
                if (bbar[i] > ub[k] + eps) { coef[k] = +1.0; cnt++; }
            }
        }
        up(E->coef, coef, (size_t)m + n);
        return cnt;
    }
    void set_orig_obj()
    {
        cbar_ok = false;
        for (int i = 1; i <= m; i++) coef[i] = 0.0;
        for (int j = 1; j <= n; j++) coef[m + j] = zeta * obj[j];
        up(E->coef, coef, (size_t)m + n);
    }
    int primal_check_stab(double tol_bnd)
    {
        for (int i = 1; i <= m; i++) {
            int k = head[i];
            if (phase == 1 && coef[k] < 0.0) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(lb[k]));
                if (bbar[i] > lb[k] + eps) return 1;
            } else if (phase == 1 && coef[k] > 0.0) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(ub[k]));
                if (bbar[i] < ub[k] - eps) return 1;
            } else {
                if (type[k] == LO || type[k] == DB || type[k] == FX) {
                    double eps = tol_bnd * (1.0 + 0.10 * std::fabs(lb[k]));
                    if (bbar[i] < lb[k] - eps) return 1;
                }
                if (type[k] == UP || type[k] == DB || type[k] == FX) {
                    double eps = tol_bnd * (1.0 + 0.10 * std::fabs(ub[k]));
                    if (bbar[i] > ub[k] + eps) return 1;
                }
            }
        }
        return 0;
    }
    int primal_check_feas(double tol_bnd)
    {
        for (int i = 1; i <= m; i++) {
            int k = head[i];
            if (coef[k] < 0.0) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(lb[k]));
                if (bbar[i] < lb[k] - eps) return 1;
            } else if (coef[k] > 0.0) {
                double eps = tol_bnd * (1.0 + 0.10 * std::fabs(ub[k]));
                if (bbar[i] > ub[k] + eps) return 1;
            }
        }
        return 0;
    }
    int primal_chuzc(double tol_dj)                       // glpspx01.js:646
    {
        down(gamma, E->gamma, n);
        sync();
        int q = 0;
        double best = 0.0;
        for (int j = 1; j <= n; j++) {
            double dj = cbar[j];
            switch (stat[j]) {
            case NL: if (dj >= -tol_dj) continue; break;
            case NU: if (dj <= +tol_dj) continue; break;
            case NF: if (-tol_dj <= dj && dj <= +tol_dj) continue; break;
            default: continue;
            }
            double temp = (dj * dj) / gamma[j];
            if (best < temp) { q = j; best = temp; }
        }
        return q;
    }
    double eval_obj()                                     // glpspx01.js:1524
    {
        double sum = obj[0];
        for (int i = 1; i <= m; i++) {
            int k = head[i];
            if (k > m) sum += obj[k - m] * bbar[i];
        }
        for (int j = 1; j <= n; j++) {
            int k = head[m + j];
            if (k > m) sum += obj[k - m] * get_xN(j);
        }
        return sum;
    }
    void store_sol(int p_stat, int d_stat, int ray)         // glpspx01.js:1591
    {
        mark("store_sol");
        pull();
        lp->valid = 1;
        f->valid = 1;
        for (int i = 1; i <= m; i++) lp->head[i] = head[i];
        lp->pbs_stat = p_stat;
        lp->dbs_stat = d_stat;
        lp->obj_val = eval_obj();
        lp->it_cnt = hs.it_cnt;
        lp->some = ray;
        // by variable (the lp arrays written in order, each variable's
        // position from bind): the values of glpspx01.js:1591-1681
        for (int k = 1; k <= m; k++) {
            const int pos = bind[k];
            const double r = lp->rii[k];
            if (pos <= m) {
                lp->row_stat[k] = BS;
                if (lp->row_bind) lp->row_bind[k] = pos;
                lp->row_prim[k] = r == 1.0 ? bbar[pos] : bbar[pos] / r;        // (x / 1 == x)
                lp->row_dual[k] = 0.0;
            } else {
                const int j = pos - m;
                const int st = stat[j];
                lp->row_stat[k] = (signed char)st;
                if (lp->row_bind) lp->row_bind[k] = 0;
                lp->row_prim[k] = st == NU ? lp->row_ub[k] : (st == NF ? 0.0 : lp->row_lb[k]);
                lp->row_dual[k] = (r == 1.0 ? cbar[j] : cbar[j] * r) / zeta;
            }
        }
        for (int c = 1; c <= n; c++) {
            const int pos = bind[m + c];
            const double q = lp->sjj[c];
            if (pos <= m) {
                lp->col_stat[c] = BS;
                if (lp->col_bind) lp->col_bind[c] = pos;
                lp->col_prim[c] = bbar[pos] * q;
                lp->col_dual[c] = 0.0;
            } else {
                const int j = pos - m;
                const int st = stat[j];
                lp->col_stat[c] = (signed char)st;
                if (lp->col_bind) lp->col_bind[c] = 0;
                lp->col_prim[c] = st == NU ? lp->col_ub[c] : (st == NF ? 0.0 : lp->col_lb[c]);
                lp->col_dual[c] = (q == 1.0 ? cbar[j] : cbar[j] / q) / zeta;
            }
        }
    }
    int fail_return()
    {
        pull();
        lp->valid = 0;
        f->valid = 0;
        lp->pbs_stat = lp->dbs_stat = 1;   // GLP_UNDEF
        lp->obj_val = 0.0;
        lp->it_cnt = hs.it_cnt;
        lp->some = 0;
        return 5;                          // GLP_EFAIL
    }

    // ---- re-inversion interval from the measured drift --------------------
    // At a re-inversion the host holds the incrementally updated values
    // (dual: cbar, primal: bbar); the fresh evaluation right after it gives
    // the drift D = max |updated - fresh| the chain accumulated.  The
    // reference's stability checks fail at tol_dj (check_stab, glpspx02.js:
    // 1410) / tol_bnd (glpspx01.js:1429) while Harris' pass 1 already relaxes
    // by 0.3 of it; the chain is halved once D > tol / 20 and doubled again
    // (up to the cap) while D < tol / 200.
    int upd_cap = 0, upd_floor = 0;
    bool drift_armed = false;
    int drift_upd = 0;
    double drift_grow = 0.0;
    std::vector<double> drift_ref;
    void drift_arm(const std::vector<double> &v, int st)
    {
        // only a re-inversion the update limit scheduled measures the chain
        // (not one after a failed pivot check or a growth check)
        drift_armed = (st == 2 && hs.upd_cnt > 0 && hs.upd_cnt >= hs.upd_lim && upd_cap > upd_floor);
        if (!drift_armed) return;
        drift_ref = v;
        drift_upd = hs.upd_cnt;
        drift_grow = hs.grow_bits ? bits_double(hs.grow_bits) : 0.0;
    }
    void drift_adapt(const std::vector<double> &fresh, int cnt, double tol)
    {
        if (!drift_armed) return;
        drift_armed = false;
        // dual: a fixed non-basic variable (NS: every DB / FX one in phase I,
        // glpspx02.js:1340-1353) has trow = 0, so its reduced cost is never
        // updated and is no part of the chain's drift (check_stab skips it)
        double D = 0.0;
        for (int j = 1; j <= cnt; j++)
            if (!dual || stat[j] != NS) D = std::max(D, std::fabs(fresh[j] - drift_ref[j]));
        // conservative in both directions: a drift above tol / 20 drops the
        // chain to the floor (nfs_max), one above tol / 100 halves it, and it
        // doubles only after two consecutive full-length chains below tol / 200
        int lim = f->upd_lim_adapt > 0 ? f->upd_lim_adapt : upd_cap;
        if (D > 0.05 * tol) {
            lim = upd_floor;
            f->clean_runs = 0;
        } else if (D > 0.01 * tol) {
            lim = std::max(upd_floor, std::min(lim, drift_upd) / 2);
            f->clean_runs = 0;
        } else if (drift_upd >= lim && ++f->clean_runs >= 2) {
            lim = std::min(upd_cap, 2 * lim);
            f->clean_runs = 0;
        }
        static const bool log = std::getenv("GK_DRIFT_LOG") != nullptr;
        if (log)
            fprintf(stderr, "[gk drift] %s it %d: %d updates, drift %.3e (tol %.1e) -> interval %d (growth checks %d, "
                    "max growth %.3e)\n", dual ? "dual" : "primal", hs.it_cnt, drift_upd, D, tol, lim, hs.echk, drift_grow);
        f->upd_lim_adapt = lim;
        hs.upd_lim = lim;
    }

    bool resident_match() const;
    void save_resident();
    bool fastv = false;                     // init took the resident arrays over (b_version)
    // move the host mirrors to / from the engine's spare set
    void swap_spare()
    {
        Engine::Spare &q = E->spare;
        type.swap(q.type); orig_type.swap(q.orig_type); stat.swap(q.stat);
        lb.swap(q.lb); ub.swap(q.ub); coef.swap(q.coef); orig_lb.swap(q.orig_lb); orig_ub.swap(q.orig_ub);
        obj.swap(q.obj); bbar.swap(q.bbar); cbar.swap(q.cbar); gamma.swap(q.gamma);
        head.swap(q.head); bind.swap(q.bind);
    }
    void init();
    void run_graph(const SpxDev &d, const DualPlan &pl, int K, int kind = 0);
    void run_graph_part(const SpxDev &d, const DualPlan &pl, int K, int kind, int part);
    bool lists_stale = false;                   // rlist / rpos / nr to rebuild from the header
    void rebuild_lists();
    void prof_events(int K)
    {
        while ((int)E->ev.size() < 4 * K) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            E->ev.push_back(e);
        }
    }
    // prof 1 / 2: per pivot t, the start / stop events of the pivot-row
    // kernel (4 t, 4 t + 1) and of the fused update kernel (4 t + 2, 4 t + 3)
    hipEvent_t ev0(int t) const { return (E->prof == 1 || E->prof == 2) ? E->ev[4 * t] : nullptr; }
    hipEvent_t ev1(int t) const { return (E->prof == 1 || E->prof == 2) ? E->ev[4 * t + 1] : nullptr; }
    hipEvent_t ev2(int t) const { return (E->prof == 1 || E->prof == 2) ? E->ev[4 * t + 2] : nullptr; }
    hipEvent_t ev3(int t) const { return (E->prof == 1 || E->prof == 2) ? E->ev[4 * t + 3] : nullptr; }
    bool ev_upd = false;                        // the last eager batch ran the fused update (its events recorded)
    int run_dual();
    int run_primal();
    int batch(int K, int rigorous);
    bool epi_arm(int K);
    void epi_wait();
    const char *epi_stage = nullptr;      // the epilogue's download in the staging ring
    // the sparse factor's Schur-correction bytes of the call's dual pivots
    // (16 m k + 8 k^2 at chain length k: Y read by the FTRAN's and the
    // BTRAN's corrections, inv(M) once), added per batch
    double sp_chain_bytes = 0.0;
};

__global__ void k_rsub_plain(double *y, const double *a, int n, const DState *st, int need_p)
{
    GATE(st, need_p);
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a[i] - y[i];
}

void Spx::rsub_into(double *y, const double *a)
{
    hipLaunchKernelGGL(k_rsub_plain, dim3((m + 255) / 256), dim3(256), 0, s, y, a, m, eg, eg ? EPI_GATE : 0);
}

__global__ void k_gather_csc_sel(int k, const int *colJ, const int *cptr, const int *crow, const double *cval,
                                 const int *rowmap, double *C, double *BS, int ms, double sign)
{
    const int b = blockIdx.x;
    const int c = colJ[b] - 1;
    for (int t = cptr[c] + threadIdx.x; t < cptr[c + 1]; t += blockDim.x) {
        const int r = crow[t];
        const int a = rowmap[r];
        const double v = sign * cval[t];
        if (a >= 0) C[(size_t)a + (size_t)b * k] = v;
        else BS[(size_t)(-a - 1) + (size_t)b * ms] = v;
    }
}

void gather_csc_sel(hipStream_t s, int k, const int *colJ, const int *cptr, const int *crow, const double *cval,
                    const int *rowmap, double *C, double *BS, int ms, double sign)
{
    if (k <= 0) return;
    hipLaunchKernelGGL(k_gather_csc_sel, dim3(k), dim3(64), 0, s, k, colJ, cptr, crow, cval, rowmap, C, BS, ms, sign);
}

int Spx::reinvert_core_csc(const BasisSplit &bs, bool refine)
{
    // structural basis columns are -A columns of the device CSC
    return reinvert_core(f, bs, nullptr, 1, -1.0, E->cptr.p, E->cind.p, E->cval.p, refine);
}

bool Spx::resident_match() const
{
    const Engine::Resident &R = E->res;
    // (fastv: init found the record valid and took its arrays, clearing ok)
    if (!(R.ok || fastv) || R.dual != dual || R.m != m || R.n != n) return false;
    if (lp->a_version == 0 || lp->a_version != R.a_version) return false;
    if (!f->valid || f->ext_upd || R.fact_ver != f->fact_ver || lists_stale) return false;
    if (std::memcmp(&R.zeta, &zeta, sizeof zeta) != 0) return false;
    auto same = [](const auto &a, const auto &b) {
        return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
    };
    // (with the bounds version the arrays are the resident ones themselves)
    if (!fastv && (!same(type, R.type) || !same(orig_type, R.orig_type) || !same(lb, R.lb) || !same(ub, R.ub) ||
                   !same(orig_lb, R.orig_lb) || !same(orig_ub, R.orig_ub) || !same(coef, R.coef) ||
                   !same(obj, R.obj)))
        return false;
    for (int i = 1; i <= m; i++)
        if (head[i] != R.head[i]) return false;
    for (int j = 1; j <= n; j++) {
        const int jo = R.bind[head[m + j]] - m;
        if (jo < 1 || jo > n || stat[j] != R.stat[jo]) return false;
    }
    return true;
}

// after a normal return: the host mirrors (current after store_sol's pull)
// become the resident record of what the device holds
void Spx::save_resident()
{
    // (the record keeps the original arrays: a return in phase I restored
    // them already, through set_orig_bnds)
    if (cur_aux) restore_orig_arrays();
    Engine::Resident &R = E->res;
    // (an epilogue result not taken up: the device holds values the mirrors
    // do not)
    R.ok = !head_stale && !vec_stale && !lists_stale && f->valid &&
           !(epi.ready && (epi.has_cbar || epi.has_bbar || epi.bounds_pending));
    if (!R.ok) return;
    R.dual = dual; R.m = m; R.n = n; R.nr = hs.nr;
    R.a_version = lp->a_version;
    R.b_version = lp->b_version;
    R.dir = lp->dir;
    R.c0 = lp->c0;
    R.fact_ver = f->fact_ver;
    R.zeta = zeta;
    R.type.swap(type); R.orig_type.swap(orig_type); R.stat.swap(stat);
    R.lb.swap(lb); R.ub.swap(ub); R.coef.swap(coef); R.orig_lb.swap(orig_lb); R.orig_ub.swap(orig_ub);
    R.obj.swap(obj); R.bbar.swap(bbar); R.cbar.swap(cbar);
    R.head.swap(head); R.bind.swap(bind);
    R.cbar_ok = cbar_ok;
    R.bbar_ok = bbar_ok;
}

void Spx::init()
{
    const double t0 = now_s();
    struct T { gk_bfd *f; double t0; ~T() { f->stats.seconds_init += now_s() - t0; } } tt{f, t0};
    const gk_lp *L = lp;
    m = L->m; n = L->n;
    s = ctx->stream;
    const size_t mn = (size_t)m + n + 1;
    swap_spare();
    // every entry 1..m+n of type / lb / ub / coef / head (1..n of obj and
    // stat) is written below: resized, not zero-filled (the spare set has the
    // size of the last call; zero-filling these arrays was most of init's
    // host time on C3); orig_* are copies of the built arrays
    // the host declares the bounds, types, costs and scale factors unchanged
    // since the call that left the resident working set (b_version, which the
    // JS shim bumps on every mutator; 0 = unknown): that call's built arrays
    // are taken over instead of rebuilt and compared (resident_match then
    // checks the basis only)
    Engine::Resident &R0 = E->res;
    fastv = L->b_version != 0 && R0.ok && R0.b_version == L->b_version && L->a_version != 0 &&
            R0.a_version == L->a_version && R0.m == m && R0.n == n && R0.dual == dual && R0.dir == L->dir &&
            std::memcmp(&R0.c0, &L->c0, sizeof(double)) == 0;
    head.resize(mn); stat.resize(n + 1);
    head[0] = 0; stat[0] = 0;
    bind.assign(mn, 0);
    gamma.resize(std::max(m, n) + 1);       // (filled by a download before every read)
    if (fastv) {
        // the record gives its arrays away here: it is no longer valid, even
        // if a check below throws before the call gets under way (a retry
        // with the same versions must rebuild, not take the spare vectors)
        R0.ok = false;
        type.swap(R0.type); orig_type.swap(R0.orig_type); lb.swap(R0.lb); ub.swap(R0.ub);
        orig_lb.swap(R0.orig_lb); orig_ub.swap(R0.orig_ub); coef.swap(R0.coef); obj.swap(R0.obj);
        zeta = R0.zeta;
    } else {
    E->auxc.ok = false;                 // the original types may have changed
    type.resize(mn); lb.resize(mn); ub.resize(mn); coef.resize(mn); obj.resize(n + 1);
    type[0] = 0; lb[0] = ub[0] = coef[0] = 0.0;
    // init_csa (glpspx01.js:42-145 / glpspx02.js:89-190)
    for (int i = 1; i <= m; i++) {
        type[i] = L->row_type[i];
        lb[i] = L->row_lb[i] * L->rii[i];
        ub[i] = L->row_ub[i] * L->rii[i];
        coef[i] = 0.0;
    }
    for (int j = 1; j <= n; j++) {
        type[m + j] = L->col_type[j];
        lb[m + j] = L->col_lb[j] / L->sjj[j];
        ub[m + j] = L->col_ub[j] / L->sjj[j];
        coef[m + j] = L->col_coef[j] * L->sjj[j];
    }
    orig_type = type; orig_lb = lb; orig_ub = ub;
    obj[0] = L->c0;
    for (int j = 1; j <= n; j++) obj[j] = coef[m + j];
    double cmax = 0.0;
    for (int j = 1; j <= n; j++)
        if (cmax < std::fabs(obj[j])) cmax = std::fabs(obj[j]);
    if (cmax == 0.0) cmax = 1.0;
    ABI_REQUIRE(L->dir == 1 || L->dir == 2, "gk_spx: dir = %d; invalid", L->dir);
    zeta = (L->dir == 1 ? +1.0 : -1.0) / cmax;
    if (std::fabs(zeta) < 1.0) zeta *= 1000.0;
    if (dual)
        for (int j = 1; j <= n; j++) coef[m + j] *= zeta;
    }
    for (int i = 1; i <= m; i++) {
        head[i] = L->head[i];
        ABI_REQUIRE(1 <= head[i] && head[i] <= m + n, "gk_spx: head[%d] = %d; out of range", i, head[i]);
    }
    int k = 0;
    for (int i = 1; i <= m; i++)
        if (L->row_stat[i] != BS) {
            k++;
            ABI_REQUIRE(k <= n, "gk_spx: too many non-basic variables");
            head[m + k] = i;
            stat[k] = L->row_stat[i];
        }
    for (int j = 1; j <= n; j++)
        if (L->col_stat[j] != BS) {
            k++;
            ABI_REQUIRE(k <= n, "gk_spx: too many non-basic variables");
            head[m + k] = m + j;
            stat[k] = L->col_stat[j];
        }
    ABI_REQUIRE(k == n, "gk_spx: basis header inconsistent with statuses (%d non-basic, n = %d)", k, n);
    for (int kk = 1; kk <= m + n; kk++) bind[head[kk]] = kk;
    static const bool ilog = std::getenv("GK_INIT_LOG") != nullptr;      // host time split of init (diagnostics)
    const double t_build = now_s();
    engine_alloc(*E, m, n, ctx);
    if (f->ext_upd) f->valid = 0;    // unit columns may be inexact after external updates
    // the working set the last call left on the device, when it is this one
    const double t_alloc = now_s();
    const bool keep = resident_match();
    kept = keep;
    const double t_match = now_s();
    Engine::Resident &R = E->res;
    R.ok = false;
    if (!keep) {
        bbar.assign(m + 1, 0.0);
        cbar.assign(n + 1, 0.0);
    }
    begin_up();
    if (!keep) {
        up(E->type, type, mn - 1); up(E->orig_type, orig_type, mn - 1);
        up(E->lb, lb, mn - 1); up(E->ub, ub, mn - 1); up(E->orig_lb, orig_lb, mn - 1); up(E->orig_ub, orig_ub, mn - 1);
        up(E->coef, coef, mn - 1); up(E->obj, obj, n);
    } else {
        // the non-basic variables are numbered as init_csa numbers them
        // (rows, then columns); the resident reduced costs follow them
        // (renumbering on the device in one workgroup, k_canon, was measured
        // 65 us per call slower than these uploads)
        cbar.resize(n + 1);
        cbar[0] = 0.0;
        for (int j = 1; j <= n; j++) cbar[j] = R.cbar[R.bind[head[m + j]] - m];
        bbar.swap(R.bbar);
        up(E->cbar, cbar, n);
    }
    up(E->head, head, mn - 1); up(E->bind, bind, mn - 1); up(E->stat, stat, n);
    flush_up();
    if (ilog)
        fprintf(stderr, "[gk init] build %.1f us, alloc %.1f us, resident check %.1f us (%s), uploads %.1f us\n",
                1e6 * (t_build - t0), 1e6 * (t_alloc - t_build), 1e6 * (t_match - t_alloc), keep ? "kept" : "rebuilt",
                1e6 * (now_s() - t_match));
    if (keep) {
        // the dense-column list of inv(B) stays as the pivots left it (its
        // order is the order of the sums over it); the PSE reference space
        // starts empty, as below
        HIPCHK(hipMemsetAsync(E->wpos.p, 0xFF, (size_t)std::max(m, n) * sizeof(int), s));
        hs = DState{};
        hs.nr = R.nr;
        hs.nwl = 0;
        cbar_ok = R.cbar_ok;
        bbar_ok = R.bbar_ok;
        f->stats.resident = 1;
    } else {
        // dense columns of inv(B): the non-basic slacks
        std::vector<int> rl, rp(m, -1);
        for (int c = 1; c <= m; c++)
            if (bind[c] > m) {
                rp[c - 1] = (int)rl.size();
                rl.push_back(c - 1);
            }
        if (!rl.empty()) HIPCHK(hipMemcpyAsync(E->rlist.p, rl.data(), rl.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(E->rpos.p, rp.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
        std::vector<int> wp(std::max(m, n), -1);   // reference space empty until the first reset (refct = 0)
        HIPCHK(hipMemcpyAsync(E->wpos.p, wp.data(), wp.size() * sizeof(int), hipMemcpyHostToDevice, s));
        hs = DState{};
        hs.nr = (int)rl.size();
        hs.nwl = 0;
        sync();
    }
    if (parm->pricing != PT_PSE) {
        // textbook pricing never resets the reference space, so nothing on
        // the device sets the weights: they are init_csa's ones (glpspx01.js:
        // 144, glpspx02.js:189), not what the last call left in the buffer
        const std::vector<double> ones(std::max(m, n), 1.0);
        HIPCHK(hipMemcpyAsync(E->gamma.p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice, s));
        sync();
    }
    hs.phase = 0;
    hs.it_cnt = L->it_cnt;
    hs.zeta = zeta;
    hs.tol_bnd = parm->tol_bnd; hs.tol_dj = parm->tol_dj; hs.tol_piv = parm->tol_piv;
    hs.obj_ll = parm->obj_ll; hs.obj_ul = parm->obj_ul;
    hs.pricing = parm->pricing; hs.rtest = parm->r_test;
    // the re-inversion interval.  The reference refactorizes after nfs_max
    // Forrest-Tomlin updates (glpfhv.js:182-187, default 100).  An explicit
    // nfs_max (any value but the default) is honoured exactly.  With the
    // default the engine may lengthen the product-form chain of the dense
    // inverse up to min(1000, m/4) — re-inversion grows with k^3 — as long as
    // the drift of the updated values against a fresh evaluation, measured at
    // every re-inversion, stays far below the tolerances the reference's own
    // checks use (drift_adapt); a chain whose drift grows is shortened
    // (BG / GR: the Schur-complement factor takes nrs_max updates before it
    // is rebuilt, glpbfd.js via lpf_create_it(nrs_max) and LPF_ELIMIT)
    const int nfs = upd_limit_parm(f->parm);
    int lim = nfs;
    if (f->parm_default) {
        // the chain starts at the cap; drift_adapt drops it to nfs_max at the
        // first measured drift above tol / 20, halves it above tol / 200 and
        // lengthens it again only after two clean full-length chains
        upd_cap = std::max(nfs, std::min(1000, m / 4));
        if (f->upd_lim_adapt <= 0) f->upd_lim_adapt = upd_cap;
        lim = std::min(std::max(f->upd_lim_adapt, nfs), upd_cap);
    } else
        upd_cap = nfs;
    if (f->sparse) {
        // the Schur-complement chain holds at most SP_KMAX updates
        // (gk_sparse.hip); under the default parameters it starts at
        // min(SP_KMAX, m/4) and drift_adapt shortens it as for the dense
        // inverse (the host L U costs ~0.1 s at m = 100,000: the interval sets
        // the amortized refactorization cost per pivot)
        if (f->parm_default) {
            upd_cap = std::min(std::max(nfs, std::min(SP_KMAX, m / 4)), SP_KMAX);
            if (f->upd_lim_adapt <= 0 || f->upd_lim_adapt > upd_cap) f->upd_lim_adapt = upd_cap;
            lim = std::min(std::max(f->upd_lim_adapt, std::min(nfs, upd_cap)), upd_cap);
        } else {
            upd_cap = std::min(nfs, SP_KMAX);
            lim = upd_cap;
        }
    }
    upd_floor = std::min(nfs, upd_cap);
    hs.upd_lim = lim;
    hs.upd_tol = f->parm.upd_tol > 0.0 ? f->parm.upd_tol : 1e-6;
    // the product-form updates of the factor persist across calls, as the
    // reference's FT eta count does in lp.bfd (glpfhv.js:182): a run of short
    // it_lim calls re-inverts on the same schedule as one long call
    hs.upd_cnt = f->valid ? std::min(f->upd_cnt, lim) : 0;
    hs.refact_pending = (f->valid && hs.upd_cnt >= lim) ? 1 : 0;
    hs.refct = 0;
    it_beg = L->it_cnt;
    tm_beg = now_s();
    push_state();
    // no wait here: the uploads are staged in the pinned ring and ordered on
    // the stream before everything the solve enqueues next
}

// The end-of-call epilogue.  A dual batch whose budget ends the call at the
// iteration limit is followed, on the host, by a fixed sequence of device
// evaluations (glpspx02.js:1614-1700 at it_lim: eval_cbar, check_stab,
// check_feas, phase I's set_orig_bnds and eval_beta, store_sol; then the next
// call's phase-I values, next_aux_launch) — each one a round of launches and
// a wait after the batch.  Enqueued here, behind the batch and before the
// host waits for it, they run on the device at once when the batch ends,
// every kernel gated on the batch having used its whole budget
// (GATE / EPI_GATE: an earlier stop leaves them no-ops and the device state
// untouched) and the list kernels reading the batch's final list length on
// the device.  The same kernels with the same inputs in the same order as the
// host sequence, so the same bits; the host sequence then takes the results
// up instead of launching (eval_cbar, set_orig_bnds, eval_bbar,
// next_aux_launch).  The paths that leave the sequence (instability, phase
// change with a re-inversion) rebuild every array the epilogue touched.
// GK_EPILOGUE=0 turns it off.
bool Spx::epi_arm(int K)
{
    const char *ev = std::getenv("GK_EPILOGUE");          // (read per call: tests switch it)
    const bool on = !ev || std::atoi(ev) != 0;
    if (!on || !dual || !E->dense || f->sparse || E->prof || (phase != 1 && phase != 2)) return false;
    if (parm->it_lim >= 0x7fffffff || hs.it_cnt - it_beg + K < parm->it_lim) return false;
    MatDev A = E->mat();
    const int nrmax = std::min(m, hs.nr + K);      // one dense column of inv(B) more or less per pivot
    if (!A.AT || !lists_ok() || nrmax > LIST_FTRAN_MAX || 2 * nrmax > m) return false;
    // (a progress line at the limit reads the batch's updated values, which
    // the epilogue replaces before the one download)
    if (f->rpt && parm->msg_lev >= 2) return false;
    const size_t region = (size_t)((const char *)(E->cbar.p + n) - (const char *)E->stm.p);
    char *stage = pin_take(region);
    if (!stage) return false;
    if (!E->epi_ev) HIPCHK(hipEventCreateWithFlags(&E->epi_ev, hipEventDisableTiming));
    eg = E->st.p;
    eg_nr = nrmax;
    eval_cbar_dev();
    if (phase == 1) {
        // check_stab / check_feas on the fresh reduced costs and the batch's
        // statuses, set_orig_bnds, and eval_beta's right-hand side split
        const size_t mn = (size_t)m + n;
        hipLaunchKernelGGL(k_epi_orig, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, s, m, n, E->orig_type.p,
                           E->orig_lb.p, E->orig_ub.p, E->bind.p, E->cbar.p, E->type.p, E->lb.p, E->ub.p, E->stat.p,
                           E->r1.p, E->wcol.p, parm->tol_dj, E->eflags.p, eg, EPI_GATE);
    }
    eval_bbar_into(dev(), E->bbar.p, phase == 1);
    // one download: the state, the check flags and head | bind | stat |
    // bbar | cbar — the batch's values when it stopped early (the epilogue
    // did nothing), the epilogue's otherwise (head and bind are the batch's
    // either way); epi_wait sorts them out
    hipLaunchKernelGGL(k_st_copy, dim3(1), dim3(64), 0, s, E->st.p, E->stm.p);
    HIPCHK(hipMemcpyAsync(stage, E->stm.p, region, hipMemcpyDeviceToHost, s));
    epi_stage = stage;
    HIPCHK(hipEventRecord(E->epi_ev, s));
    // the next call's phase-I values (next_aux_launch) behind the wait point
    const char *ea = std::getenv("GK_NEXT_AUX");
    const bool aux_on = !ea || std::atoi(ea) != 0;
    epi.aux = (phase == 1 && aux_on);
    if (epi.aux) next_aux_dev();
    eg = nullptr;
    epi.has_cbar = epi.has_bbar = true;
    epi.bounds_pending = (phase == 1);
    epi.checks = (phase == 1);
    return true;
}

void Spx::epi_wait()
{
    HIPCHK(hipEventSynchronize(E->epi_ev));
    f->stats.host_syncs++;
    for (const Pending &q : pending) std::memcpy(q.dst, q.src, q.bytes);
    pending.clear();
    const char *lo = (const char *)E->stm.p;
    auto at = [&](const void *dev) { return epi_stage + ((const char *)dev - lo); };
    std::memcpy(&hs, epi_stage, sizeof(DState));
    std::memcpy(head.data() + 1, at(E->head.p), ((size_t)m + n) * sizeof(int));
    std::memcpy(bind.data() + 1, at(E->bind.p), ((size_t)m + n) * sizeof(int));
    std::memcpy(stat.data() + 1, at(E->stat.p), (size_t)n);
    std::memcpy(bbar.data() + 1, at(E->bbar.p), (size_t)m * sizeof(double));
    std::memcpy(cbar.data() + 1, at(E->cbar.p), (size_t)n * sizeof(double));
    if (hs.stop <= ST_BATCH) {
        // the epilogue ran: the mirrors hold its values (eval_cbar, phase
        // I's set_orig_bnds and eval_beta), which the host sequence takes up
        // in its own order (eval_cbar, set_orig_bnds, eval_bbar); the checks
        // on the batch's statuses came from the device (eflags)
        epi.stat.assign(stat.begin(), stat.end());
        if (epi.checks) {
            const int *fl = (const int *)at(E->eflags.p);
            int sf = 0, ff = 0;
            for (int b = 0; b < (m + n + 255) / 256; b++) {
                sf |= fl[2 * b];
                ff |= fl[2 * b + 1];
            }
            epi.stab = sf;
            epi.feas = ff;
        }
    }
    pin_off = 0;
}

int Spx::batch(int K, int rigorous)
{
    mark("batch");
    const double t0 = now_s();
    const int k_chain0 = hs.upd_cnt;
    struct T { gk_bfd *f; double t0; ~T() { f->stats.seconds_batches += now_s() - t0; } } tt{f, t0};
    epi_drop();
    bool armed = false;
    hs.stop = ST_RUN;
    std::memset(hs.gate, 0, sizeof hs.gate);   // (0 between launches; a clean start whatever a failed run left)
    hs.iter_left = K;
    hs.npiv = 0;
    hs.phase = phase;
    hs.rigorous = rigorous;
    hs.dinf = 0;
    hs.pend = 0;
    push_state();
    if (dual && E->dense && (E->pnl_m != m || E->pnl_n != n)) {
        // the pricing panel's buffers; no slot is valid until a fill (pslot
        // entries are validated against ppos)
        const int ldp = (n + 7) & ~7;
        E->pnl.ensure((size_t)PANEL_MAX * ldp);
        E->pnl_src.ensure((size_t)PANEL_MAX * m);
        E->pslot.ensure(m);
        E->ppos.ensure(PANEL_MAX);
        HIPCHK(hipMemsetAsync(E->pslot.p, 0xff, (size_t)m * sizeof(int), s));
        HIPCHK(hipMemsetAsync(E->ppos.p, 0, PANEL_MAX * sizeof(int), s));
        E->pnl_m = m;
        E->pnl_n = n;
    }
    SpxDev d = dev();
    const int pse = (parm->pricing == PT_PSE);
    if (dual) {
        // plans are bucketed so that a handful of captured graphs serve a solve
        auto bucket = [](int x, int cap) {
            int g = std::max(64, x / 8);
            return std::min(cap, (x + g - 1) / g * g);
        };
        // the cap of the list follows the list, not the budget: nr moves by
        // far less than one per pivot, and a cap sized for K more entries
        // loses the fused update (nr_cap + 2 <= 256) and widens every
        // speculative list load long before the list needs it.  A batch that
        // does reach its cap stops with ST_CAP and is planned again
        // (run_dual).  GK_PLAN_SLACK (read per call: tests switch it) is the
        // slack; at least 1, so the first pivot of a batch always runs
        const char *es = std::getenv("GK_PLAN_SLACK");
        const int slack = std::max(1, es ? std::atoi(es) : 32);
        int nr_cap = std::min(bucket(hs.nr + slack, m), bucket(hs.nr + K + 1, m));
        // the bucket that crosses the fused update's limit is clipped to it
        if (nr_cap > DUAL_UPDATE_NR_MAX && hs.nr + slack <= DUAL_UPDATE_NR_MAX) nr_cap = DUAL_UPDATE_NR_MAX;
        DualPlan pl = dual_plan(d, nr_cap, bucket(hs.nwl + K + 1, n), pse, rigorous);
        pl.sparse = f->sparse ? 1 : 0;
        // profiling launches eagerly: event-record nodes inside captured
        // graphs are not timed by every HIP runtime this library may bind to
        // prof 1/2 launch eagerly (events around the pivot-row kernel); prof 3
        // keeps the graphs and records only the per-block clock stamps
        const int evp = E->prof == 1 || E->prof == 2;
        if (evp) prof_events(K);
        // sharded: the RCCL exchange is a stream operation and is captured
        // with the pivot's kernels (so are the simulated ranks'); the TCP
        // exchange goes through the host and keeps the batch eager
        const bool shard_eager = d.shard && d.shard->vsize <= 1 && gk_comm_backend(d.shard->comm) != GK_COMM_RCCL;
        if (d.shard) d.shard->exchanges += K;    // (every launched pivot exchanges, a stopped one too)
        static const bool no_graph = [] {      // GK_NO_GRAPH=1 (diagnostics): every batch eager
            const char *e = std::getenv("GK_NO_GRAPH");
            return e && std::atoi(e) != 0;
        }();
        if (!rigorous && K >= 4 && !evp && !f->sparse && !shard_eager && !no_graph) {
            run_graph(d, pl, K);
            armed = epi_arm(K);
        } else {
            dual_batch_begin(s, d, pl);
            for (int t = 0; t < K; t++) dual_iteration2(s, d, pl, ev0(t), ev1(t), ev2(t), ev3(t));
            dual_batch_end(s, d, pl);
            ev_upd = evp && pl.fupd && pl.rowpath;
        }
    } else if (f->sparse) {
        // the primal pivot on the sparse factor (rigorous mode included: no
        // refinement, the checks re-factorize as after any failure)
        primal_batch_begin(s, d);
        for (int t = 0; t < K; t++) primal_iteration_sparse(s, d, pse);
    } else if (!rigorous && primal_fast_ok(d)) {
        if (lists_stale) {
            rebuild_lists();
            d = dev();
        }
        auto bucket = [](int x, int cap) {
            int g = std::max(64, x / 8);
            return std::min(cap, (x + g - 1) / g * g);
        };
        const DualPlan pl = primal_plan(d, bucket(hs.nr + K + 1, m), pse);
        if (K >= 4) run_graph(d, pl, K, 1);
        else {
            primal_batch_begin(s, d);
            for (int t = 0; t < K; t++) primal_iteration2(s, d, pl);
        }
    } else {
        for (int t = 0; t < K; t++) primal_iteration(s, d, pse, rigorous);
        lists_stale = true;                   // the single-workgroup kernels do not maintain rlist
    }
    mark("batch launched");
    if (armed) epi_wait();
    else pull_state();
    mark("batch done");
    f->stats.batches++;
    f->stats.pivots += hs.npiv;
    if (dual && f->sparse)
        for (int i = 0; i < hs.npiv; i++) {
            const double k = (double)(k_chain0 + i);
            sp_chain_bytes += 16.0 * (double)m * k + 8.0 * k * k;
        }
    f->stats.bytes_pivots = hs.bytes + sp_chain_bytes;
    f->stats.trow_bytes = hs.bytes_trow;
    f->stats.trow_dev_ms = hs.trow_ticks / (double)ctx->wall_khz;
    f->stats.trow_dev_ms_b = hs.trow_ticks_b / (double)ctx->wall_khz;
    f->stats.trow_dev_launches = (long long)hs.trow_n;
    f->stats.trow_dev_ms_r = hs.trow_ticks_r / (double)ctx->wall_khz;
    f->stats.trow_dev_launches_r = (long long)hs.trow_nr;
    if (E->prof != 1 && E->prof != 2) {                 // (prof 1 / 2: the update's events, below)
        f->stats.upd_dev_ms = hs.upd_ticks / (double)ctx->wall_khz;
        f->stats.upd_dev_launches = (long long)hs.upd_n;
    }
    f->stats.upd_bytes = hs.bytes_upd;
    f->stats.panel_hits = (long long)hs.phits;
    f->stats.panel_refills = (long long)hs.pmisses;
    if (dual && (E->prof == 1 || E->prof == 2)) {
        for (int t = 0; t < hs.npiv; t++) {
            float ms = 0.f;
            hipError_t e = hipEventElapsedTime(&ms, E->ev[4 * t], E->ev[4 * t + 1]);
            if (e != hipSuccess)
                throw AbiError{std::string("event timing: ") + hipGetErrorName(e) + " t=" + std::to_string(t) +
                               " K=" + std::to_string(K) + " npiv=" + std::to_string(hs.npiv) +
                               " graph=" + std::to_string(!rigorous && K >= 4) + " nev=" + std::to_string(E->ev.size()) +
                               " q0=" + hipGetErrorName(hipEventQuery(E->ev[4 * t])) +
                               " q1=" + hipGetErrorName(hipEventQuery(E->ev[4 * t + 1]))};
            f->stats.trow_ms += ms;
            f->stats.trow_launches++;
            // the fused update's events (the same extended launch); with
            // prof 1 / 2 these fields carry them instead of clock stamps
            if (ev_upd && hipEventElapsedTime(&ms, E->ev[4 * t + 2], E->ev[4 * t + 3]) == hipSuccess) {
                f->stats.upd_dev_ms += ms;
                f->stats.upd_dev_launches++;
            }
        }
    }
    // (armed: the mirrors were downloaded behind the batch, before the
    // epilogue changed anything)
    if (armed) head_stale = vec_stale = false;
    if (hs.npiv > 0) {
        if (!armed) head_stale = vec_stale = true;
        cbar_ok = bbar_ok = false;
    }
    if (armed && hs.stop <= ST_BATCH) {
        ABI_REQUIRE(hs.nr <= eg_nr, "spx: list length %d beyond the epilogue's bound %d", hs.nr, eg_nr);
        epi.ready = true;
    } else
        epi_drop();
    // a stop on the budget leaves the top kernel of the next iteration unrun
    return hs.stop == ST_RUN ? ST_BATCH : hs.stop;
}

// rlist / rpos (the dense columns of inv(B): the non-basic slacks) from the
// header, after batches of the single-workgroup primal kernels
void Spx::rebuild_lists()
{
    pull();
    cbar_ok = bbar_ok = false;                  // the list order sets the order of the sums
    std::vector<int> rl, rp(m, -1);
    for (int c = 1; c <= m; c++)
        if (bind[c] > m) {
            rp[c - 1] = (int)rl.size();
            rl.push_back(c - 1);
        }
    if (!rl.empty()) HIPCHK(hipMemcpyAsync(E->rlist.p, rl.data(), rl.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(E->rpos.p, rp.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s));
    hs.nr = (int)rl.size();
    // the basic slacks in the PSE reference space (the support of u = inv(B)' v
    // beyond the dense columns, gk_primal.hip)
    std::vector<signed char> ref((size_t)m + n);
    HIPCHK(hipMemcpyAsync(ref.data(), E->refsp.p, (size_t)m + n, hipMemcpyDeviceToHost, s));
    sync();
    std::vector<int> sl, sp(std::max(m, n), -1);
    for (int c = 1; c <= m; c++)
        if (bind[c] <= m && ref[c - 1]) {
            sp[c - 1] = (int)sl.size();
            sl.push_back(c - 1);
        }
    if (!sl.empty()) HIPCHK(hipMemcpyAsync(E->wlist.p, sl.data(), sl.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(E->wpos.p, sp.data(), sp.size() * sizeof(int), hipMemcpyHostToDevice, s));
    hs.nwl = (int)sl.size();
    push_state();
    sync();
    lists_stale = false;
}

// A batch of K pivots is one captured graph — or, from K = 32 on, two: a
// head of 8 pivots and the rest.  hipGraphLaunch submits a graph's kernels
// from the host before the device runs the first of them (≈140 µs for the
// ≈300 kernels of a 100-pivot batch, GK_CALL_LOG): the device starts on the
// head after ≈12 µs and runs it while the host submits the tail.  The
// kernel sequence is the same either way.
void Spx::run_graph(const SpxDev &d, const DualPlan &pl, int K, int kind)
{
    static const int head = [] {
        const char *e = std::getenv("GK_GRAPH_HEAD");
        return e ? std::atoi(e) : 8;
    }();
    if (head > 0 && K >= 32 && K > head) {
        run_graph_part(d, pl, head, kind, 1);
        run_graph_part(d, pl, K - head, kind, 2);
    } else
        run_graph_part(d, pl, K, kind, 0);
}

// part 0: the whole batch; 1: its head (batch begin, no end); 2: its tail
void Spx::run_graph_part(const SpxDev &d, const DualPlan &pl, int K, int kind, int part)
{
    Engine &En = *E;
    GraphEntry *hit = nullptr;
    const int key = kind | (part << 4);
    for (auto &g : En.graphs)
        if (g.K == K && g.kind == key && std::memcmp(&g.pl, &pl, sizeof(pl)) == 0 &&
            std::memcmp(&g.d, &d, sizeof(d)) == 0) {
            hit = &g;
            break;
        }
    if (!hit) {
        hipGraph_t graph = nullptr;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        if (kind == 0) {
            if (part != 2) dual_batch_begin(s, d, pl);
            for (int t = 0; t < K; t++) dual_iteration2(s, d, pl);
            if (part != 1) dual_batch_end(s, d, pl);
        } else {
            if (part != 2) primal_batch_begin(s, d);
            for (int t = 0; t < K; t++) primal_iteration2(s, d, pl);
        }
        HIPCHK(hipStreamEndCapture(s, &graph));
        hipGraphExec_t exec = nullptr;
        HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
        (void)hipGraphDestroy(graph);
        if (En.graphs.size() >= 24) {          // evict the least recently used
            auto lru = std::min_element(En.graphs.begin(), En.graphs.end(),
                                        [](const GraphEntry &a, const GraphEntry &b) { return a.last < b.last; });
            (void)hipGraphExecDestroy(lru->exec);
            En.graphs.erase(lru);
        }
        GraphEntry g;
        g.d = d; g.pl = pl; g.K = K; g.kind = key; g.exec = exec;
        En.graphs.push_back(g);
        hit = &En.graphs.back();
        f->stats.graphs_built++;
    }
    hit->last = ++En.graph_clock;
    HIPCHK(hipGraphLaunch(hit->exec, s));
}

// pivots per device batch: doubled while batches end on their budget, back
// to the minimum after any other stop (a stop drains the rest of the batch)
// (a stop on the plan's cap is no trouble: the size stays)
static int next_batch(int k, int why) { return why == ST_BATCH ? std::min(2 * k, 64) : (why == ST_CAP ? k : 8); }

// a batch that would run past the update limit stops inside its graph and
// drains the rest as gated no-op launches: end it at the re-inversion point
// instead, in power-of-two steps (their graphs are cached) down to 8
static int align_to_refactor(int K, int left)
{
    if (left <= 0 || left >= K) return K;
    if (left < 8) return left;
    int p = 8;
    while (2 * p <= left) p *= 2;
    return p;
}

int Spx::run_dual()
{
    const gk_smcp *P = parm;
    int binv_st = f->valid ? 2 : 0, bbar_st = 0, cbar_st = 0, rigorous = 0;
    int ret;
    for (;;) {
        if (binv_st == 0) {
            pull();
            drift_arm(cbar, cbar_st);
            const long long nref0 = f->stats.refinements;
            if (!reinvert()) {
                report_msg(GK_MSG_FACTERR, 1, fact_ret);     // GLP_MSG_ERR
                return fail_return();
            }
            det_log(f->stats.refinements != nref0 ? "reinv-newton" : "reinv");
            binv_st = 1;
            bbar_st = cbar_st = 0;
            hs.upd_cnt = sp_replayed; hs.refact_pending = 0; hs.grow_bits = 0;
        }
        hs.binv_fresh = (binv_st == 1);
        int feas_pre = -1;                 // phase I: check_feas of this iteration, found with check_stab
        if (cbar_st == 0) {
            dinf_known = false;
            pull();
            eval_cbar();
            drift_adapt(cbar, n, P->tol_dj);
            cbar_st = 1;
            bool sel_aux = false;
            if (phase == 0) {
                mark("phase sel");
                if (dual_check_feas(0.90 * P->tol_dj) != 0) { phase = 1; set_aux_bnds(); sel_aux = true; }
                else { phase = 2; set_orig_bnds(); }
                mark("bounds set");
                hs.refct = 0;
                bbar_st = 0;
            }
            // check_stab (glpspx02.js:1410).  Right after set_aux_bnds every
            // status follows the sign of its reduced cost (NL: d >= 0, NU:
            // d < 0, NS), so it cannot fail there; in phase I the same pass
            // gives check_feas (:1296), which the phase-I test below takes
            int stab_fail = 0;
            if (sel_aux) stab_fail = 0;
            else if (phase == 1 && epi.ready && epi.checks && !epi.has_cbar) {
                // (the epilogue's checks: the cbar just taken up and the
                // statuses the batch left)
                stab_fail = epi.stab;
                feas_pre = epi.feas;
                epi.checks = false;
            } else if (phase == 1) stab_fail = dual_check_stab_feas(P->tol_dj, &feas_pre);
            else stab_fail = dual_check_stab(P->tol_dj);
            mark("stab checked");
            if (stab_fail != 0) {
                static const bool dlog = std::getenv("GK_DRIFT_LOG") != nullptr;
                if (dlog) {
                    double worst = 0.0;
                    int cnt = 0;
                    for (int j = 1; j <= n; j++) {
                        const double v = (stat[j] == NL) ? -cbar[j] : (stat[j] == NU) ? cbar[j]
                                         : (stat[j] == NF) ? std::fabs(cbar[j]) : 0.0;
                        if (v > P->tol_dj) { cnt++; worst = std::max(worst, v); }
                    }
                    fprintf(stderr, "[gk drift] dual it %d: check_stab failed, %d reduced costs off by up to %.3e "
                            "(%d updates since the last re-inversion)\n", hs.it_cnt, cnt, worst, hs.upd_cnt);
                }
                report_msg(GK_MSG_INSTAB, 1, 2);
                if (P->meth == 2) {            // GLP_DUALP
                    store_sol(1, 1, 0);
                    return 5;
                }
                phase = 0;
                binv_st = 0;
                rigorous = 5;
                continue;
            }
        }
        if (phase == 1) {
            // check_feas: the last pivot's commit evaluated it on the device
            // when the batch ran to its budget
            int infeas;
            if (dinf_known) infeas = hs.dinf;
            else if (feas_pre >= 0) infeas = feas_pre;
            else {
                pull();
                infeas = dual_check_feas(P->tol_dj);
            }
            if (infeas == 0) {
                pull();
                display(1);
                phase = 2;
                if (cbar_st != 1) { eval_cbar(); cbar_st = 1; }
                set_orig_bnds();
                hs.refct = 0;
                bbar_st = 0;
            }
        }
        if (bbar_st == 0) {
            pull();
            eval_bbar();
            if (phase == 2) hs.obj = eval_obj();
            bbar_st = 1;
        }
        hs.cbar_fresh = (cbar_st == 1);
        if (phase == 2 && zeta < 0.0 && P->obj_ll > -DBL_MAX && hs.obj <= P->obj_ll) {
            if (bbar_st != 1 || cbar_st != 1) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                continue;
            }
            display(1);
            report_msg(GK_MSG_OBJLL, 3);
            store_sol(3, 2, 0);
            return 6;                                  // GLP_EOBJLL
        }
        if (phase == 2 && zeta > 0.0 && P->obj_ul < +DBL_MAX && hs.obj >= P->obj_ul) {
            if (bbar_st != 1 || cbar_st != 1) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                continue;
            }
            display(1);
            report_msg(GK_MSG_OBJUL, 3);
            store_sol(3, 2, 0);
            return 7;                                  // GLP_EOBJUL
        }
        {
            bool it_hit = P->it_lim < 0x7fffffff && hs.it_cnt - it_beg >= P->it_lim;
            bool tm_hit = !it_hit && P->tm_lim < 0x7fffffff && 1000.0 * (now_s() - tm_beg) >= P->tm_lim;
            // (column-sharded pricing: every rank must stop on the same pivot,
            // so the wall-clock decision is taken collectively — any rank's)
            if (!it_hit && P->tm_lim < 0x7fffffff && f->shard && E->dense && !f->sparse)
                tm_hit = shard_any(*f->shard, tm_hit);
            if (it_hit || tm_hit) {
                if ((phase == 2 && bbar_st != 1) || cbar_st != 1) {
                    if (phase == 2 && bbar_st != 1) bbar_st = 0;
                    if (cbar_st != 1) cbar_st = 0;
                    continue;
                }
                mark("it_lim");
                display(1);
                report_msg(it_hit ? GK_MSG_ITLIM : GK_MSG_TMLIM, 3);
                mark("reported");
                int d_stat;
                const int ph = phase;
                if (phase == 1) {
                    pull();
                    d_stat = 3;
                    set_orig_bnds();
                    mark("orig bounds");
                    eval_bbar();
                } else
                    d_stat = 2;
                store_sol(3, d_stat, 0);
                mark("stored");
                if (ph == 1) {
                    phase = 1;                     // the phase the next call resumes in
                    mark("next_aux");
                    next_aux_launch();
                    mark("next_aux launched");
                }
                return it_hit ? 8 : 9;
            }
        }
        if (hs.refact_pending && binv_st != 0) {
            // the update limit was reached at the end of the last batch:
            // re-invert before launching (a batch would stop at its first pivot)
            binv_st = 0;
            refine_next = (hs.echk == echk_seen);
            continue;
        }
        display(0);
        int K = rigorous ? 1 : E->kbatch;
        if (P->it_lim < 0x7fffffff) {
            // an iteration budget of up to two full batches runs as one
            const int rem = P->it_lim - (hs.it_cnt - it_beg);
            K = (!rigorous && K >= 64 && rem <= 128) ? rem : std::max(1, std::min(K, rem));
        }
        K = align_to_refactor(K, hs.upd_lim - hs.upd_cnt);
        K = ahead_align(K);
        K = align_to_display(K);
        int why = batch(K, rigorous);
        if (f->sparse) ahead_maybe();
        det_log("batch", K, why);
        if (f->sparse) sp_stamps_dump(*f->sp, s, ctx->wall_khz);
        E->kbatch = next_batch(E->kbatch, why);
        dinf_known = (why == ST_BATCH && hs.npiv > 0);
        if (hs.npiv > 0) {
            bbar_st = 2;
            cbar_st = 2;
            binv_st = 2;
            rigorous = hs.rigorous;
        }
        switch (why) {
        case ST_BATCH:
        case ST_PHASE:
        case ST_OBJLIM:
        case ST_CAP:        // the list reached the plan's cap: the next batch is planned from the new nr
            break;
        case ST_REFACT:
            binv_st = 0;
            refine_next = (hs.echk == echk_seen);
            break;
        case ST_P0:
            if (bbar_st != 1 || cbar_st != 1) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                break;
            }
            {
                display(1);
                report_msg(phase == 1 ? GK_MSG_NODFS : GK_MSG_OPTIMAL, 3);
                int p_stat, d_stat;
                if (phase == 1) {
                    pull();
                    set_orig_bnds();
                    eval_bbar();
                    p_stat = 3; d_stat = 4;
                } else
                    p_stat = d_stat = 2;
                store_sol(p_stat, d_stat, 0);
            }
            return 0;
        case ST_Q0:
            if (bbar_st != 1 || cbar_st != 1 || !rigorous) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                rigorous = 1;
                break;
            }
            display(1);
            if (phase == 1) {
                report_msg(GK_MSG_NOCHOICE, 1);
                return fail_return();
            }
            report_msg(GK_MSG_NOPFS, 3);
            pull();
            store_sol(4, 2, head[hs.p]);
            return 0;
        case ST_SMALLPIV:
            rigorous = 5;
            break;
        case ST_PIVCHK:
            if (binv_st != 1) binv_st = 0;
            rigorous = 5;
            break;
        default:
            throw AbiError{"spx_dual: unexpected device stop code"};
        }
        (void)ret;
    }
}

int Spx::run_primal()
{
    const gk_smcp *P = parm;
    int binv_st = f->valid ? 2 : 0, bbar_st = 0, cbar_st = 0, rigorous = 0;
    for (;;) {
        if (binv_st == 0) {
            pull();
            drift_arm(bbar, bbar_st);
            const long long nref0 = f->stats.refinements;
            if (!reinvert()) {
                report_msg(GK_MSG_FACTERR, 1, fact_ret);     // GLP_MSG_ERR
                return fail_return();
            }
            det_log(f->stats.refinements != nref0 ? "reinv-newton" : "reinv");
            binv_st = 1;
            bbar_st = cbar_st = 0;
            hs.upd_cnt = sp_replayed; hs.refact_pending = 0; hs.grow_bits = 0;
        }
        hs.binv_fresh = (binv_st == 1);
        if (bbar_st == 0) {
            pull();
            eval_bbar();
            drift_adapt(bbar, m, P->tol_bnd);
            bbar_st = 1;
            if (phase == 0) {
                if (set_aux_obj(P->tol_bnd) > 0) phase = 1;
                else { set_orig_obj(); phase = 2; }
                ABI_REQUIRE(primal_check_stab(P->tol_bnd) == 0, "spx_primal: check_stab after phase selection");
                cbar_st = 0;
                display(1);
            }
            if (primal_check_stab(P->tol_bnd)) {
                report_msg(GK_MSG_INSTAB, 1, 1);
                phase = 0;
                binv_st = 0;
                rigorous = 5;
                continue;
            }
        }
        if (phase == 1) {
            pull();
            if (!primal_check_feas(P->tol_bnd)) {
                phase = 2;
                set_orig_obj();
                cbar_st = 0;
                display(1);
            }
        }
        if (cbar_st == 0) {
            pull();
            eval_cbar();
            cbar_st = 1;
        }
        hs.cbar_fresh = (cbar_st == 1);
        {
            bool it_hit = P->it_lim < 0x7fffffff && hs.it_cnt - it_beg >= P->it_lim;
            bool tm_hit = !it_hit && P->tm_lim < 0x7fffffff && 1000.0 * (now_s() - tm_beg) >= P->tm_lim;
            if (it_hit || tm_hit) {
                if (bbar_st != 1 || (phase == 2 && cbar_st != 1)) {
                    if (bbar_st != 1) bbar_st = 0;
                    if (phase == 2 && cbar_st != 1) cbar_st = 0;
                    continue;
                }
                display(1);
                report_msg(it_hit ? GK_MSG_ITLIM : GK_MSG_TMLIM, 3);
                int p_stat;
                pull();
                if (phase == 1) {
                    p_stat = 3;
                    set_orig_obj();
                    eval_cbar();
                } else
                    p_stat = 2;
                int q = primal_chuzc(P->tol_dj);
                store_sol(p_stat, q == 0 ? 2 : 3, 0);
                return it_hit ? 8 : 9;
            }
        }
        if (hs.refact_pending && binv_st != 0) {
            // the update limit was reached at the end of the last batch:
            // re-invert before launching (a batch would stop at its first pivot)
            binv_st = 0;
            refine_next = (hs.echk == echk_seen);
            continue;
        }
        display(0);
        int K = rigorous ? 1 : E->kbatch;
        if (P->it_lim < 0x7fffffff) {
            // an iteration budget of up to two full batches runs as one
            const int rem = P->it_lim - (hs.it_cnt - it_beg);
            K = (!rigorous && K >= 64 && rem <= 128) ? rem : std::max(1, std::min(K, rem));
        }
        K = align_to_refactor(K, hs.upd_lim - hs.upd_cnt);
        K = ahead_align(K);
        K = align_to_display(K);
        int why = batch(K, rigorous);
        if (f->sparse) ahead_maybe();
        det_log("batch", K, why);
        E->kbatch = next_batch(E->kbatch, why);
        if (hs.npiv > 0) {
            bbar_st = 2;
            rigorous = hs.rigorous;
            // cbar and the factor change only on basis changes; the device keeps
            // their freshness flags, mirror them here
            if (!hs.cbar_fresh) cbar_st = 2;
            if (!hs.binv_fresh) binv_st = 2;
        }
        switch (why) {
        case ST_BATCH:
        case ST_PHASE:
            break;
        case ST_REFACT:
            binv_st = 0;
            refine_next = (hs.echk == echk_seen);
            break;
        case ST_Q0:
            if (bbar_st != 1 || cbar_st != 1) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                break;
            }
            {
                display(1);
                report_msg(phase == 1 ? GK_MSG_NOPFS : GK_MSG_OPTIMAL, 3);
                int p_stat, d_stat;
                pull();
                if (phase == 1) {
                    p_stat = 4;
                    set_orig_obj();
                    eval_cbar();
                    int q = primal_chuzc(P->tol_dj);
                    d_stat = (q == 0 ? 2 : 3);
                } else
                    p_stat = d_stat = 2;
                store_sol(p_stat, d_stat, 0);
            }
            return 0;
        case ST_DCHK:
            if (cbar_st != 1) cbar_st = 0;
            rigorous = 5;
            break;
        case ST_P0:
            if (bbar_st != 1 || cbar_st != 1 || !rigorous) {
                if (bbar_st != 1) bbar_st = 0;
                if (cbar_st != 1) cbar_st = 0;
                rigorous = 1;
                break;
            }
            display(1);
            if (phase == 1) {
                report_msg(GK_MSG_NOCHOICE, 1);
                return fail_return();
            }
            report_msg(GK_MSG_UNBND, 3);
            pull();
            store_sol(2, 4, head[m + hs.q]);
            return 0;
        case ST_SMALLPIV:
            rigorous = 5;
            break;
        case ST_PIVCHK:
            if (binv_st != 1) binv_st = 0;
            rigorous = 5;
            break;
        default:
            throw AbiError{"spx_primal: unexpected device stop code"};
        }
    }
}

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------
extern "C" {

int gk_abi_version(void) { return GK_ABI_VERSION; }

const char *gk_last_error(void) { return g_err.c_str(); }

int gk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

gk_ctx *gk_ctx_create(int device)
{
    try {
        int cnt = 0;
        HIPCHK(hipGetDeviceCount(&cnt));
        ABI_REQUIRE(device >= 0 && device < cnt, "gk_ctx_create: device %d of %d", device, cnt);
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, device));
        ABI_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0,
                    "gk_ctx_create: device %d is %s; this build targets gfx950 (MI355X) only", device, prop.gcnArchName);
        HIPCHK(hipSetDevice(device));
        gk_ctx *c = new gk_ctx;
        c->device = device;
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
            c->wall_khz = khz;
        return c;
    } catch (const AbiError &e) {
        g_err = e.msg;
        return nullptr;
    }
}

void gk_ctx_destroy(gk_ctx *ctx)
{
    if (!ctx) return;
    ctx_unref(ctx);
}

gk_bfd *gk_bfd_create(gk_ctx *ctx)
{
    if (!ctx) { set_err("gk_bfd_create: null context"); return nullptr; }
    gk_bfd *f = new gk_bfd;
    f->ctx = ctx;
    ctx->refs++;
    // glp_get_bfcp defaults (glpapi12.js:111-121)
    f->parm.type = 1; f->parm.lu_size = 0; f->parm.piv_tol = 0.10; f->parm.piv_lim = 4; f->parm.suhl = 1;
    f->parm.eps_tol = 1e-15; f->parm.max_gro = 1e10; f->parm.nfs_max = 100; f->parm.upd_tol = 1e-6;
    f->parm.nrs_max = 100; f->parm.rs_size = 0;
    return f;
}

void gk_bfd_destroy(gk_bfd *f)
{
    if (!f) return;
    (void)hipSetDevice(f->ctx->device);
    if (f->ctx->stream) (void)hipStreamSynchronize(f->ctx->stream);
    delete f->eng;
    delete f->shard;
    if (f->sp) sp_destroy(f->sp);
    f->Binv.release(); f->C.release(); f->X.release(); f->Y.release(); f->CinvR.release(); f->BS.release();
    f->G.release(); f->vecx.release(); f->vecy.release(); f->partial.release(); f->idx_i.release();
    f->piv_step.release(); f->piv.release(); f->flag.release(); f->bptr.release(); f->brow.release(); f->bval.release();
    gk_ctx *ctx = f->ctx;
    delete f;
    ctx_unref(ctx);
}

// the checks of glp_set_bfcp (glpapi12.js:133-166), messages included (the
// rs_size message prints nrs_max there too); type FT / BG / GR all select the
// explicit-inverse factor, the fields of the sparse LU (piv_tol, piv_lim,
// suhl, lu_size, eps_tol, max_gro, nrs_max, rs_size) are kept but steer
// nothing; nfs_max and upd_tol act (re-inversion interval, update check)
int gk_bfd_set_parm(gk_bfd *f, const gk_bfcp *parm)
{
    if (!f || !parm) { set_err("gk_bfd_set_parm: null argument"); return GK_EABI; }
    const gk_bfcp &b = *parm;
    if (!(b.type == 1 || b.type == 2 || b.type == 3)) { set_err("glp_set_bfcp: type = %d; invalid parameter", b.type); return GK_EABI; }
    if (b.lu_size < 0) { set_err("glp_set_bfcp: lu_size = %d; invalid parameter", b.lu_size); return GK_EABI; }
    if (!(0.0 < b.piv_tol && b.piv_tol < 1.0)) { set_err("glp_set_bfcp: piv_tol = %.17g; invalid parameter", b.piv_tol); return GK_EABI; }
    if (b.piv_lim < 1) { set_err("glp_set_bfcp: piv_lim = %d; invalid parameter", b.piv_lim); return GK_EABI; }
    if (!(b.suhl == 1 || b.suhl == 0)) { set_err("glp_set_bfcp: suhl = %d; invalid parameter", b.suhl); return GK_EABI; }
    if (!(0.0 <= b.eps_tol && b.eps_tol <= 1e-6)) { set_err("glp_set_bfcp: eps_tol = %.17g; invalid parameter", b.eps_tol); return GK_EABI; }
    if (b.max_gro < 1.0) { set_err("glp_set_bfcp: max_gro = %.17g; invalid parameter", b.max_gro); return GK_EABI; }
    if (!(1 <= b.nfs_max && b.nfs_max <= 32767)) { set_err("glp_set_bfcp: nfs_max = %d; invalid parameter", b.nfs_max); return GK_EABI; }
    if (!(0.0 < b.upd_tol && b.upd_tol < 1.0)) { set_err("glp_set_bfcp: upd_tol = %.17g; invalid parameter", b.upd_tol); return GK_EABI; }
    if (!(1 <= b.nrs_max && b.nrs_max <= 32767)) { set_err("glp_set_bfcp: nrs_max = %d; invalid parameter", b.nrs_max); return GK_EABI; }
    if (b.rs_size < 0) { set_err("glp_set_bfcp: rs_size = %d; invalid parameter", b.nrs_max); return GK_EABI; }
    f->parm = b;
    if (f->parm.rs_size == 0) f->parm.rs_size = 20 * f->parm.nrs_max;
    // explicit parameters (glp_set_bfcp with a parm): nfs_max / nrs_max are
    // honoured exactly, whatever their value — 100 included
    f->parm_default = false;
    f->upd_lim_adapt = 0;
    f->clean_runs = 0;
    return 0;
}

// glp_set_bfcp(lp, NULL) (glpapi12.js:135-139) / a factor whose problem has
// no bfcp of its own: the defaults of glp_get_bfcp, with the re-inversion
// interval left to the engine's drift measurement (gk_engine.hip drift_adapt)
int gk_bfd_reset_parm(gk_bfd *f)
{
    if (!f) { set_err("gk_bfd_reset_parm: null argument"); return GK_EABI; }
    f->parm.type = 1; f->parm.lu_size = 0; f->parm.piv_tol = 0.10; f->parm.piv_lim = 4; f->parm.suhl = 1;
    f->parm.eps_tol = 1e-15; f->parm.max_gro = 1e10; f->parm.nfs_max = 100; f->parm.upd_tol = 1e-6;
    f->parm.nrs_max = 100; f->parm.rs_size = 0;
    f->parm_default = true;
    f->upd_lim_adapt = 0;
    f->clean_runs = 0;
    return 0;
}

int gk_bfd_valid(const gk_bfd *f) { return f ? f->valid : 0; }

void gk_bfd_set_report(gk_bfd *f, gk_report_fn fn, void *ud)
{
    if (!f) return;
    f->rpt = fn;
    f->rpt_ud = ud;
}

int gk_bfd_get_count(const gk_bfd *f)
{
    if (!f || !f->valid) { set_err("bfd_get_count: factorization is not valid"); return GK_EABI; }
    return f->upd_cnt;
}

void gk_bfd_last_stats(const gk_bfd *f, gk_spx_stats *st)
{
    if (f && st) *st = f->stats;
}

void gk_bfd_profile(gk_bfd *f, int enable)
{
    if (f) f->prof = (enable >= 2 && enable <= 4) ? enable : (enable ? 1 : 0);
}

int gk_bfd_trace(gk_bfd *f, unsigned long long *out, size_t cnt)
{
    if (!f || !out || !f->eng || !f->eng->trace.p) return 0;
    const size_t nn = std::min(cnt, f->eng->trace.n);
    if (hipMemcpy(out, f->eng->trace.p, nn * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return (int)nn;
}

// Which factor a solve runs on.  The explicit inverse
// serves dense A (the row path over AT, the MFMA panel and re-inversion) and
// small or dense-basis LPs.  Sparse A takes the sparse LU (gk_sparse.hip)
// beyond the inverse's limit (m > 65535) and whenever the basis is both large
// and sparse: the inverse costs 8 m^2 bytes, a rank-1 pass over m x nr of them
// per pivot and O(k^3) re-inversions, against level sweeps over the LU's
// entries — on the block-angular m = 4,005 LP 7.7k against 3.2k pivots/s
// (profiles/r04_sparse_blocks40*).  col_nnz: the average entries per column
// of A (a solve) or of B (glp_factorize without a resident problem).
// GK_SPARSE=1 / 0 force one (0 only up to m = 65535); GK_SPARSE_MIN_M moves
// the size threshold (default 2048).
static int factor_choice(int m, double col_nnz, bool dense)
{
    const char *ev = std::getenv("GK_SPARSE");
    const int want = ev ? std::atoi(ev) : -1;
    if (dense) return 0;
    if (m > 65535 || want == 1) return 1;
    if (want == 0) return 0;
    static const int min_m = [] {
        const char *e = std::getenv("GK_SPARSE_MIN_M");
        return e ? std::max(1, std::atoi(e)) : 2048;
    }();
    return (m >= min_m && 16.0 * col_nnz <= (double)m) ? 1 : 0;
}

static void bfd_prepare(gk_bfd *f, int m)
{
    HIPCHK(hipSetDevice(f->ctx->device));
    if (f->m != m) {
        f->m = m;
        f->ldb = (m + 7) & ~7;
        f->valid = 0;
    }
}

int gk_bfd_factorize_csc(gk_bfd *f, int m, const int *ptr, const int *ind, const double *val)
{
    try {
        ABI_REQUIRE(f && m >= 1, "bfd_factorize: m = %d; invalid parameter", m);
        bfd_prepare(f, m);
        f->valid = 0;
        hipStream_t s = f->ctx->stream;
        // the factor spx_entry would choose, so that a glp_factorize of an
        // advanced basis before glp_simplex is the factor the solve then
        // uses: by the resident problem's A when there is one, else by the
        // density of B itself (a mismatch only costs the solve a re-factor)
        const Engine *E0 = f->eng;
        const bool known = E0 && E0->m == m && E0->n > 0;
        const long long nnzb = (long long)ptr[m + 1] - ptr[1];
        const int sparse = known ? factor_choice(m, (double)E0->nnz / E0->n, E0->dense != 0)
                                 : factor_choice(m, (double)nnzb / m, false);
        if (sparse) {
            for (int j = 1; j <= m; j++) {
                const int len = ptr[j + 1] - ptr[j];
                ABI_REQUIRE(0 <= len && len <= m, "luf_factorize: j = %d; len = %d; invalid column length", j, len);
                for (int p = ptr[j]; p < ptr[j + 1]; p++) {
                    ABI_REQUIRE(1 <= ind[p] && ind[p] <= m, "luf_factorize: i = %d; j = %d; invalid row index", ind[p],
                                j);
                    ABI_REQUIRE(val[p] != 0.0, "luf_factorize: i = %d; j = %d; zero element not allowed", ind[p], j);
                }
            }
            if (!f->sp) f->sp = sp_create();
            f->sparse = 1;
            int ret;
            try {
                ret = sp_factorize_csc(*f->sp, s, m, ptr, ind, val, f->parm.piv_tol, f->parm.piv_lim, f->parm.eps_tol);
            } catch (const std::exception &e) {
                throw AbiError{e.what()};
            }
            f->fact_ver++;
            f->valid = ret == 0;
            f->upd_cnt = 0;
            f->ext_upd = 0;
            return ret ? 1 : 0;   // BFD_ESING
        }
        f->sparse = 0;                       // the explicit inverse (glp_factorize's factor)
        // classify unit columns (+1 on a single row) as slack-like
        BasisSplit bs;
        std::vector<int> srow_pos(m + 1, 0), cptr(m + 1), crow, colJ_all;
        std::vector<double> cval;
        std::vector<char> isslack(m + 1, 0);
        for (int j = 1; j <= m; j++) {
            int len = ptr[j + 1] - ptr[j];
            ABI_REQUIRE(0 <= len && len <= m, "luf_factorize: j = %d; len = %d; invalid column length", j, len);
            if (len == 1 && val[ptr[j]] == 1.0 && !srow_pos[ind[ptr[j]]]) {
                int r = ind[ptr[j]];
                ABI_REQUIRE(1 <= r && r <= m, "luf_factorize: i = %d; j = %d; invalid row index", r, j);
                srow_pos[r] = j;
                isslack[j] = 1;
            }
        }
        int t = 0;
        for (int j = 1; j <= m; j++) {
            cptr[j - 1] = t;
            std::vector<char> seen;
            for (int p = ptr[j]; p < ptr[j + 1]; p++) {
                int r = ind[p];
                ABI_REQUIRE(1 <= r && r <= m, "luf_factorize: i = %d; j = %d; invalid row index", r, j);
                ABI_REQUIRE(val[p] != 0.0, "luf_factorize: i = %d; j = %d; zero element not allowed", r, j);
                crow.push_back(r - 1);
                cval.push_back(val[p]);
                t++;
            }
            if (!isslack[j]) { bs.posJ.push_back(j); bs.colJ.push_back(j); }
        }
        cptr[m] = t;
        bs.rowmap.assign(m, 0);
        for (int r = 1; r <= m; r++) {
            if (srow_pos[r]) {
                bs.rowmap[r - 1] = -(int)(bs.rowS.size() + 1);
                bs.rowS.push_back(r);
                bs.posS.push_back(srow_pos[r]);
            } else {
                bs.rowmap[r - 1] = (int)bs.rowR.size();
                bs.rowR.push_back(r);
            }
        }
        bs.k = (int)bs.posJ.size();
        bs.ms = (int)bs.rowS.size();
        ABI_REQUIRE(bs.k == (int)bs.rowR.size(), "bfd_factorize: basis classification failed");
        f->bptr.ensure(m + 1);
        f->brow.ensure(std::max(t, 1));
        f->bval.ensure(std::max(t, 1));
        HIPCHK(hipMemcpyAsync(f->bptr.p, cptr.data(), (m + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (t) {
            HIPCHK(hipMemcpyAsync(f->brow.p, crow.data(), t * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(f->bval.p, cval.data(), t * sizeof(double), hipMemcpyHostToDevice, s));
        }
        int ret = reinvert_core(f, bs, nullptr, 1, 1.0, f->bptr.p, f->brow.p, f->bval.p);
        return ret ? 1 : 0;   // BFD_ESING
    } catch (const AbiError &e) {
        g_err = e.msg;
        return GK_EABI;
    }
}

int gk_bfd_factorize(gk_bfd *f, int m, gk_col_fn col, void *info)
{
    try {
        ABI_REQUIRE(f && m >= 1 && col, "bfd_factorize: m = %d; invalid parameter", m);
        std::vector<int> ptr(m + 2), ind(1), tind(m + 1);
        std::vector<double> val(1), tval(m + 1);
        ptr[1] = 1;
        ind.reserve((size_t)4 * m + 1);
        val.reserve((size_t)4 * m + 1);
        for (int j = 1; j <= m; j++) {
            int len = col(info, j, tind.data(), tval.data());
            ABI_REQUIRE(0 <= len && len <= m, "luf_factorize: j = %d; len = %d; invalid column length", j, len);
            for (int t = 1; t <= len; t++) { ind.push_back(tind[t]); val.push_back(tval[t]); }
            ptr[j + 1] = ptr[j] + len;
        }
        return gk_bfd_factorize_csc(f, m, ptr.data(), ind.data(), val.data());
    } catch (const AbiError &e) {
        g_err = e.msg;
        return GK_EABI;
    }
}

static void bfd_solve(gk_bfd *f, double *x, int tr)
{
    ABI_REQUIRE(f && f->valid, "bfd_%stran: factorization is not valid", tr ? "b" : "f");
    HIPCHK(hipSetDevice(f->ctx->device));
    hipStream_t s = f->ctx->stream;
    const int m = f->m;
    f->vecx.ensure(m);
    f->vecy.ensure(m);
    f->partial.ensure(PARTIAL_CAP);
    HIPCHK(hipMemcpyAsync(f->vecx.p, x + 1, m * sizeof(double), hipMemcpyHostToDevice, s));
    if (f->sparse) {
        try {
            if (tr) sp_btran(*f->sp, s, f->vecx.p, f->vecy.p);
            else sp_ftran(*f->sp, s, f->vecx.p, f->vecy.p);
        } catch (const std::exception &e) {
            throw AbiError{e.what()};
        }
    } else if (tr) gemv_t(s, f->Binv.p, m, m, f->ldb, f->vecx.p, f->vecy.p, 1.0);
    else gemv_n(s, f->Binv.p, m, m, f->ldb, f->vecx.p, f->partial.p, PARTIAL_CAP, f->vecy.p, 1.0, nullptr, 0.0);
    HIPCHK(hipMemcpyAsync(x + 1, f->vecy.p, m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
}

void gk_bfd_ftran(gk_bfd *f, double *x)
{
    try { bfd_solve(f, x, 0); } catch (const AbiError &e) { g_err = e.msg; }
}

void gk_bfd_btran(gk_bfd *f, double *x)
{
    try { bfd_solve(f, x, 1); } catch (const AbiError &e) { g_err = e.msg; }
}

int gk_bfd_update(gk_bfd *f, int j, int len, const int *ind, int idx, const double *val)
{
    try {
        ABI_REQUIRE(f && f->valid, "bfd_update_it: factorization is not valid");
        const int m = f->m;
        ABI_REQUIRE(1 <= j && j <= m, "fhv_update_it: j = %d; column number out of range", j);
        if (f->upd_cnt >= upd_limit_parm(f->parm)) { f->valid = 0; return 4; }  // BFD_ELIMIT
        // the sparse factor's updates are the engine's own (Schur complement on
        // the device); an external update asks for a refactorization instead
        if (f->sparse) { f->valid = 0; return 4; }
        HIPCHK(hipSetDevice(f->ctx->device));
        hipStream_t s = f->ctx->stream;
        std::vector<double> a(m + 1, 0.0);
        for (int k = 1; k <= len; k++) {
            int i = ind[idx + k];
            ABI_REQUIRE(1 <= i && i <= m, "fhv_update_it: ind[%d] = %d; row number out of range", k, i);
            ABI_REQUIRE(a[i] == 0.0, "fhv_update_it: ind[%d] = %d; duplicate row index not allowed", k, i);
            ABI_REQUIRE(val[k] != 0.0, "fhv_update_it: val[%d] = 0; zero element not allowed", k);
            a[i] = val[k];
        }
        f->vecx.ensure(m);
        f->vecy.ensure(m);
        f->G.ensure(m);
        f->partial.ensure(PARTIAL_CAP);
        HIPCHK(hipMemcpyAsync(f->vecx.p, a.data() + 1, m * sizeof(double), hipMemcpyHostToDevice, s));
        // t = -inv(B) a (the tcol convention of the rank-1 kernel)
        gemv_n(s, f->Binv.p, m, m, f->ldb, f->vecx.p, f->partial.p, PARTIAL_CAP, f->vecy.p, -1.0, nullptr, 0.0);
        std::vector<double> t(m + 1);
        HIPCHK(hipMemcpyAsync(t.data() + 1, f->vecy.p, m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        double big = 0.0;
        for (int i = 1; i <= m; i++) big = std::max(big, std::fabs(t[i]));
        if (t[j] == 0.0) { f->valid = 0; return 1; }                                  // BFD_ESING
        if (std::fabs(t[j]) < f->parm.upd_tol * big) { f->valid = 0; return 3; }      // BFD_ECHECK
        gather_row(s, f->Binv.p, f->ldb, m, j, f->G.p);
        binv_rank1(s, f->Binv.p, m, f->ldb, f->G.p, f->vecy.p, j);
        HIPCHK(hipStreamSynchronize(s));
        f->upd_cnt++;
        f->fact_ver++;
        f->ext_upd = 1;
        return 0;
    } catch (const AbiError &e) {
        g_err = e.msg;
        return GK_EABI;
    }
}

static int spx_entry(gk_ctx *ctx, gk_lp *lp, gk_bfd *f, const gk_smcp *parm, int dual)
{
    try {
        ABI_REQUIRE(ctx && lp && f && parm, "gk_spx: null argument");
        ABI_REQUIRE(lp->m > 0 && lp->n > 0, "spx: m = %d, n = %d; invalid dimensions", lp->m, lp->n);
        HIPCHK(hipSetDevice(ctx->device));
        if (f->ctx != ctx) {                  // the factor moves to the caller's context
            ctx->refs++;
            ctx_unref(f->ctx);
            f->ctx = ctx;
        }
        const double t0 = now_s();
        f->stats = gk_spx_stats{};
        bfd_prepare(f, lp->m);
        if (!f->eng) f->eng = new Engine;
        f->eng->prof = f->prof;
        engine_upload_matrix(f, lp);
        // the factor: the explicit inverse, or the sparse LU with Schur-
        // complement updates (gk_sparse.hip), both simplex methods, as
        // factor_choice decides
        {
            const bool big = lp->m > 65535;
            const int sp = factor_choice(lp->m, (double)f->eng->nnz / std::max(1, f->eng->n), f->eng->dense != 0);
            ABI_REQUIRE(sp || !big, "spx: m = %d exceeds the explicit inverse's limit 65535 (sparse A: the sparse "
                        "factor serves m > 65535)", lp->m);
            if (sp != f->sparse) {
                f->valid = 0;
                f->sparse = sp;
            }
            if (sp && !f->sp) f->sp = sp_create();
            f->stats.factor_sparse = sp;
        }
        if (f->shard && (f->shard->n != f->eng->n || f->shard->m != f->eng->m)) {
            // the exchange's buffers for this n: slices of L = ceil(n / size),
            // then max |trow| and the A w partial (m) — L + 1 + m doubles a rank
            LpShard &sh = *f->shard;
            const int n = f->eng->n, m = f->eng->m;
            const int parts = sh.vsize > 1 ? sh.vsize : sh.size;
            sh.L = (n + parts - 1) / parts;
            const size_t blk = (size_t)sh.L + 1 + (size_t)m;
            if (sh.dsend) (void)hipFree(sh.dsend);
            if (sh.drecv) (void)hipFree(sh.drecv);
            sh.dsend = sh.drecv = nullptr;
            HIPCHK(hipMalloc((void **)&sh.dsend, blk * sizeof(double)));
            HIPCHK(hipMalloc((void **)&sh.drecv, (size_t)parts * blk * sizeof(double)));
            sh.hsend.assign(blk, 0.0);
            sh.hrecv.assign((size_t)sh.size * blk, 0.0);
            sh.n = n;
            sh.m = m;
        }
        const long long shard_ex0 = f->shard ? f->shard->exchanges : 0;
        Spx S;
        S.ctx = ctx; S.f = f; S.E = f->eng; S.lp = lp; S.parm = parm; S.dual = dual;
        S.mark("entry");
        S.init();
        S.mark("init done");
        lp->valid = 0;
        int ret = dual ? S.run_dual() : S.run_primal();
        S.mark("run done");
        f->upd_cnt = S.hs.upd_cnt;
        f->stats.evals_skipped = S.evals_skipped;
        if (f->shard) f->stats.shard_exchanges = f->shard->exchanges - shard_ex0;
        if (ret == 0 || (ret >= 6 && ret <= 9)) S.save_resident();
        S.swap_spare();
        S.mark("exit");
        f->stats.seconds_total = now_s() - t0;
        if (!S.marks.empty()) {
            std::string line = "[gk call]";
            char buf[64];
            for (auto &mk : S.marks) {
                std::snprintf(buf, sizeof buf, " %s %.1f", mk.first, 1e6 * (mk.second - S.marks[0].second));
                line += buf;
            }
            fprintf(stderr, "%s\n", line.c_str());
        }
        return ret;
    } catch (const AbiError &e) {
        g_err = e.msg;
        if (f && f->shard) shard_abort(*f->shard);
        return GK_EABI;
    } catch (const std::exception &e) {
        g_err = e.what();
        if (f && f->shard) shard_abort(*f->shard);
        return GK_EABI;
    }
}

int gk_spx_primal(gk_ctx *ctx, gk_lp *lp, gk_bfd *bfd, const gk_smcp *parm) { return spx_entry(ctx, lp, bfd, parm, 0); }

// column-sharded pricing: the dual on this factor forms each
// pivot row from this rank's slice of the non-basic positions and gathers
// the others' over comm; every rank of comm must make the same calls on the
// same problem.  comm = NULL (or a communicator of one rank) turns it off
int gk_bfd_set_comm(gk_bfd *f, gk_comm *comm)
{
    try {
        ABI_REQUIRE(f, "gk_bfd_set_comm: null factor");
        delete f->shard;
        f->shard = nullptr;
        if (!comm) return 0;
        int rank = 0;
        const int size = gk_comm_size_rank(comm, &rank);
        static const bool one_rank = [] {          // test knob: the exchange with one rank
            const char *e = std::getenv("GK_SHARD_ONE_RANK");
            return e && std::atoi(e) != 0;
        }();
        if (size < 1 || (size == 1 && !one_rank)) return 0;
        f->shard = new LpShard;
        f->shard->comm = comm;
        f->shard->rank = rank;
        f->shard->size = size;
        if (size == 1) {                            // (read per call: measurements switch it)
            const char *e = std::getenv("GK_SHARD_SIM");
            f->shard->vsize = e ? std::max(0, std::min(std::atoi(e), 64)) : 0;
        }
        return 0;
    } catch (const AbiError &e) {
        g_err = e.msg;
        return GK_EABI;
    }
}

int gk_spx_dual(gk_ctx *ctx, gk_lp *lp, gk_bfd *bfd, const gk_smcp *parm) { return spx_entry(ctx, lp, bfd, parm, 1); }

}  // extern "C"

namespace gk {
// gk_mip.hip's fallback for a node LP the batched kernel could not finish:
// glp_simplex with meth = GLP_DUALP (solve_lp, glpapi06.js:27-37) on a fresh
// factorization of lp->head
int gk_spx_node(gk_ctx *ctx, gk_lp *lp, gk_bfd *bfd, const gk_smcp *parm)
{
    if (bfd) bfd->valid = 0;
    int ret = spx_entry(ctx, lp, bfd, parm, 1);
    if (ret == 5 && lp->valid) ret = spx_entry(ctx, lp, bfd, parm, 0);
    return ret;
}
}  // namespace gk

// u[t * m + pos[t]] = 1 (the unit right-hand sides of the batched BTRANs)
__global__ void k_unit_rows(double *u, int m, int nk, const int *pos)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nk) u[(size_t)t * m + pos[t]] = 1.0;
}

extern "C" int gk_bfd_eval_tab_rows(gk_bfd *f, gk_lp *lp, int nk, const int *k, double *alfa, int flags)
{
    try {
        ABI_REQUIRE(f && lp && (nk == 0 || (k && alfa)), "glp_eval_tab_row: null argument");
        ABI_REQUIRE(lp->m > 0 && lp->n > 0 && nk >= 0, "glp_eval_tab_row: m = %d, n = %d, nk = %d", lp->m, lp->n, nk);
        ABI_REQUIRE(f->valid && f->m == lp->m, "glp_eval_tab_row: basis factorization does not exist");
        if (nk == 0) return 0;
        HIPCHK(hipSetDevice(f->ctx->device));
        const int m = lp->m, n = lp->n;
        // basis positions (glp_get_row_bind / glp_get_col_bind) and the SB
        // entry of each requested row
        std::vector<int> bind(m + n + 1, 0), pos(nk);
        for (int i = 1; i <= m; i++) {
            ABI_REQUIRE(1 <= lp->head[i] && lp->head[i] <= m + n, "glp_eval_tab_row: head[%d] out of range", i);
            bind[lp->head[i]] = i;
        }
        std::vector<double> rs(nk), cs(n), aux(m);
        for (int t = 0; t < nk; t++) {
            const int kk = k[t];
            ABI_REQUIRE(1 <= kk && kk <= m + n, "glp_eval_tab_row: k = %d; variable number out of range", kk);
            ABI_REQUIRE(bind[kk] != 0, "glp_eval_tab_row: k = %d; variable must be basic", kk);
            pos[t] = bind[kk] - 1;
            rs[t] = kk <= m ? 1.0 / lp->rii[kk] : lp->sjj[kk - m];
        }
        for (int j = 1; j <= n; j++) cs[j - 1] = lp->col_stat[j] == BS ? 0.0 : 1.0 / lp->sjj[j];
        for (int i = 1; i <= m; i++) aux[i - 1] = lp->row_stat[i] == BS ? 0.0 : -lp->rii[i];
        if (!f->eng) f->eng = new Engine;
        engine_upload_matrix(f, lp);
        hipStream_t s = f->ctx->stream;
        const size_t ldo = (size_t)m + n;
        DBuf<double> G, sc, out;
        DBuf<int> dpos;
        struct Rel {
            DBuf<double> &a, &b, &c;
            DBuf<int> &d;
            ~Rel() { a.release(); b.release(); c.release(); d.release(); }
        } rel{G, sc, out, dpos};
        G.ensure((size_t)nk * m);
        sc.ensure((size_t)nk + n + m);
        out.ensure((size_t)nk * ldo);
        dpos.ensure(nk);
        HIPCHK(hipMemcpyAsync(dpos.p, pos.data(), nk * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.p, rs.data(), nk * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.p + nk, cs.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(sc.p + nk + n, aux.data(), m * sizeof(double), hipMemcpyHostToDevice, s));
        if (f->sparse) {
            // the rows of inv(B) by BTRANs of e_pos on the sparse factor
            // (glp_eval_tab_row's own glp_btran, glpapi12.js:430), then the
            // same products with A
            DBuf<double> units;                     // e_pos of every row, on the stream (no host copies in between)
            units.ensure((size_t)nk * m);
            fill_d(s, units.p, 0.0, (size_t)nk * m);
            hipLaunchKernelGGL(k_unit_rows, dim3((nk + 63) / 64), dim3(64), 0, s, units.p, m, nk, dpos.p);
            for (int t = 0; t < nk; t++) {
                try {
                    sp_btran(*f->sp, s, units.p + (size_t)t * m, G.p + (size_t)t * m);
                } catch (const std::exception &e) {
                    throw AbiError{e.what()};
                }
            }
            HIPCHK(hipStreamSynchronize(s));
            units.release();
        }
        tab_rows(s, f->sparse ? nullptr : f->Binv.p, f->ldb, f->eng->mat(), nk, dpos.p, G.p, sc.p + nk + n, sc.p + nk,
                 sc.p, out.p, (flags & 1) ? 0 : 1);
        HIPCHK(hipGetLastError());
        // through a pinned buffer of our own: a direct copy into the host's
        // array leaves that (pageable, host-runtime-owned) memory registered
        // with the HIP runtime, and a host that frees it at exit (node's
        // heap teardown) then faults
        const size_t bytes = (size_t)nk * ldo * sizeof(double);
        void *pin = nullptr;
        HIPCHK(hipHostMalloc(&pin, bytes, hipHostMallocDefault));
        const hipError_t ce = hipMemcpyAsync(pin, out.p, bytes, hipMemcpyDeviceToHost, s);
        const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(s) : ce;
        if (se == hipSuccess) std::memcpy(alfa, pin, bytes);
        (void)hipHostFree(pin);
        HIPCHK(se);
        return 0;
    } catch (const AbiError &e) {
        g_err = e.msg;
        return GK_EABI;
    }
}

extern "C" double gk_bfd_time_kernel(gk_bfd *f, int which, int reps, double *bytes)
{
    try {
        ABI_REQUIRE(f && f->eng && f->valid && reps > 0, "gk_bfd_time_kernel: no resident problem");
        HIPCHK(hipSetDevice(f->ctx->device));
        Engine &E = *f->eng;
        hipStream_t s = f->ctx->stream;
        const int m = E.m, n = E.n;
        MatDev A = E.mat();
        double *scratch = nullptr;
        double b = 0.0;
        const double vec = 8.0;
        DState hst{};
        HIPCHK(hipMemcpyAsync(&hst, E.st.p, sizeof(DState), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        SpxDev d{};
        d.m = m; d.n = n; d.A = A; d.st = E.st.p; d.rho_idx = E.rho_idx.p; d.rho_val = E.rho_val.p;
        d.partial = E.partial.p; d.partial_cap = PARTIAL_CAP;
        const DualPlan pl = dual_plan(d, hst.ns, 0, 0, 0);
        const bool rows = (which == 0 && pl.rowpath && hst.ns > 0);
        switch (which) {
        case 0:
            b = rows ? 8.0 * (double)hst.ns * n + 12.0 * hst.ns
                     : (A.dense ? 8.0 * m * (double)n : 12.0 * E.nnz) + vec * (m + 2.0 * n) + 4.0 * (m + n) + n;
            break;
        case 1: b = (A.dense ? 8.0 * m * (double)n : 12.0 * E.nnz) + vec * (n + 2.0 * m); break;
        case 2: b = 8.0 * m * (double)m + vec * 2.0 * m; break;
        case 3: b = 16.0 * m * (double)m + vec * 2.0 * m; break;
        default: ABI_REQUIRE(false, "gk_bfd_time_kernel: which = %d", which);
        }
        if (which == 3) {
            HIPCHK(hipMalloc((void **)&scratch, (size_t)f->ldb * m * sizeof(double)));
            HIPCHK(hipMemcpyAsync(scratch, f->Binv.p, (size_t)f->ldb * m * sizeof(double), hipMemcpyDeviceToDevice, s));
            fill_d(s, E.tcol.p, 1.0, m);
        }
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        auto launch = [&]() {
            switch (which) {
            case 0:
                if (rows) launch_trow_rows(s, d, pl, hst.ns);
                else colpass(s, A, CP_TROW, m, n, E.head.p, E.stat.p, E.coef.p, nullptr, E.rho.p, nullptr, E.trow.p,
                             nullptr, nullptr);
                break;
            case 1: aprod_neg(s, A, E.wcol.p, E.ys.p, E.work.p, E.partial.p, PARTIAL_CAP); break;
            case 2: gemv_n(s, f->Binv.p, m, m, f->ldb, E.h.p, E.partial.p, PARTIAL_CAP, E.tcol.p, 1.0, nullptr, 0.0); break;
            case 3: binv_rank1(s, scratch, m, f->ldb, E.rowp.p, E.tcol.p, 1); break;
            }
        };
        launch();                               // warm
        if (which == 1 || which == 2) fill_d(s, which == 1 ? E.wcol.p : E.h.p, 1.0, which == 1 ? n : m);
        HIPCHK(hipEventRecord(e0, s));
        for (int r = 0; r < reps; r++) launch();
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (scratch) (void)hipFree(scratch);
        if (bytes) *bytes = b;
        return (double)ms / reps;
    } catch (const AbiError &err) {
        g_err = err.msg;
        return -1.0;
    }
}

// accessors for the other translation units (gk_mip.hip)
__global__ void k_gk_mark(int tag, int *sink)
{
    if (tag < 0 && sink) sink[0] = tag;      // never taken: the launch itself is the marker
}

int gk_ctx_mark(gk_ctx *c, int tag)
{
    if (!c) return GK_EABI;
    hipLaunchKernelGGL(k_gk_mark, dim3(1), dim3(64), 0, c->stream, tag, (int *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : GK_EABI;
}

int gk_ctx_device(gk_ctx *c) { return c->device; }
void mip_cache_free_hook(void *p);
void **gk_ctx_mip_cache(gk_ctx *c, void (**freer)(void *))
{
    c->mip_cache_free = mip_cache_free_hook;
    *freer = mip_cache_free_hook;
    return &c->mip_cache;
}
void gk_ios_set_report(gk_ctx *c, gk_report_fn fn, void *ud)
{
    if (!c) return;
    c->ios_rpt = fn;
    c->ios_rpt_ud = ud;
}
void gk_ctx_ios_report(gk_ctx *c, gk_report_fn *fn, void **ud)
{
    *fn = c ? c->ios_rpt : nullptr;
    *ud = c ? c->ios_rpt_ud : nullptr;
}
hipStream_t gk_ctx_stream(gk_ctx *c) { return c->stream; }
namespace gk {
void set_err(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
}  // namespace gk
