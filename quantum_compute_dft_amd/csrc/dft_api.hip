// C-ABI of libdft.so (include/dft_solver.h) and the host orchestration behind it.
//
// Replaces src/dft_solver.cu:530-719 of the reference (XCSolver classes, the
// per-call cudaMalloc/cudaFree sequence and the four extern "C" entry points).
// Differences by design: one persistent workspace per solver instead of 6-7
// allocations per call; 64-bit index arithmetic; deterministic reductions;
// errors are recorded (DFT_GetLastError) as well as printed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dft_solver.h"
#include "ao_kernels.hpp"
#include "jk_kernels.hpp"
#include "cd_kernels.hpp"
#include "cd_response_kernels.hpp"
#include "xc_big_kernels.hpp"
#include "xc_ws_kernels.hpp"
#include "xc_kernels.hpp"
#include "xc_occ_launch.hpp"
#include "xc_tiny_launch.hpp"
#include "dm_factor_launch.hpp"
#include "xc_response_launch.hpp"
#include "xc_response_pol_launch.hpp"
#include "xc_spin_launch.hpp"
#include "xc_grad_launch.hpp"
#include "becke_launch.hpp"
#include "xc_meta_launch.hpp"
#include "xc_meta_spin_launch.hpp"
#include "xc_grad_meta_launch.hpp"
#include "xc_grad_meta_spin_launch.hpp"

using namespace qcdft;

namespace {

// One device allocation, sized by reserve().  It frees itself with its owner: DFT_DestroySolver deletes the solver on the
// solver's device after the stream has drained, so no list of the solver's buffers is kept anywhere.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    double *d() const { return (double *)p; }
};

struct Timing {
    const char *name;
    hipEvent_t t0, t1;
};

// The arguments of a sweep, and with them the key of a recorded one
struct SweepArgs {
    long ngrid;
    int nao, nocc;
    const double *dm, *ao, *grad, *w;
    double *vxc;
    const double *cocc;
    bool operator==(const SweepArgs &o) const
    {
        return ngrid == o.ngrid && nao == o.nao && nocc == o.nocc && dm == o.dm && ao == o.ao && grad == o.grad && w == o.w &&
               vxc == o.vxc && cocc == o.cocc;
    }
};

// One recorded sweep (option "graph"): the launches of a call with exactly these arguments, replayed as one HIP graph.
struct SweepGraph {
    SweepArgs key = {};
    hipGraphExec_t exec = nullptr;
    int seen = 0;      // calls with this key so far (the first sizes the workspace, the second is recorded)
    bool bad = false;  // recording failed once: this key runs as plain launches from then on
    unsigned long stamp = 0;
};

// The planes of one sweep, reserved together (reserve_planes): the density, its gradient (3 per point) and sigma, the
// coefficient planes that the pointwise kernel leaves for the contraction, and that kernel's Exc partials.
struct Planes {
    DevBuf rho, grad, sigma, coef, partial;
};

// One prepared response of Vxc: the weighted derivative table of the functional at the ground-state density and that
// density's gradient (g0[1]: the beta gradient, open-shell slot only), kept between a Prepare and its Applies in buffers
// nothing else writes.
struct FxcSlot {
    DevBuf table, g0[2];
    long ngrid = 0;   // what the table was prepared for (0: nothing prepared, or invalidated)
    int nao = 0;
};

} // namespace

struct XCSolver {
    int type = 0;
    bool needs_grad = false;     // the functional reads grad rho: four planes, ao_grad required (every type but LDA and LDA-class mixes)
    xc::MixWeights mix = {};     // SOLVER_MIX: the eight coefficients, fixed at creation (recorded graphs hold them)
    // DFT_CreateSolverMeta: the two meta-GGA coefficients.  meta_active (one is non-zero): the functional reads tau, which only
    // DFT_ComputeXCMeta forms -- every other XC entry refuses the solver (enter)
    bool is_meta = false, meta_active = false;
    double meta[2] = {0.0, 0.0};
    hipStream_t stream = nullptr;
    bool device_ok = false;
    int device = 0; // the device that was current at DFT_CreateSolver: every entry point runs there
    int num_cu = 256;
    // options
    int quirks = 1;
    int path = 0; // 0 auto (wave-specialised persistent kernels when nao <= 128), 1 VALU validation, 2 generic MFMA
    int profile = 0;
    int ksplit = 0;
    int ao_pt = 0; // grid points per workgroup of the AO kernel: 0 auto, 8 or 16
    // 0 (default): Exc is finished by a one-block kernel of its own BEHIND the Vxc reduce -- stream order puts it after
    // every store of the call, so the host-mapped word means "the whole call has completed" for any consumer (other
    // streams, mapped host reads): the reference's contract (blocking copy + cudaFree, dft_solver.cu:575-582).
    // 1 (opt-in): the reduce kernel's highest-index block finishes Exc itself (one launch and ~1.5 us fewer); the word
    // then only orders consumers on the solver's own stream.
    int fuse_finish = 0;
    int sweep_order = 2; // bit 0: rho kernel walks the grid backwards, bit 1: Vxc kernel does (default: rho forward, Vxc backward)
    int tiny = -1;     // one-pass sweep kernel for nao <= 32 (xc_tiny_kernels.hpp): -1 auto (where it is faster, tiny_pays()), 0 off, 1 on
    int occ = 0;       // DFT_ComputeXCOcc: 0 auto (occupied-orbital density step where it does fewer MFMAs), 1 always, 2 never
    int used_occ = 0;  // what the last sweep did (DFT_GetTimings names say so too)
    // DFT_ComputeXC / DFT_ComputeXC64 (a dm and no orbitals): 1 = factorise dm on the device (dm_factor.hip) and sweep with the
    // factor as occupied orbitals where the "occ" rule takes that form; 0 (default, or QCDFT_DM_FACTOR=1 in the environment
    // at DFT_CreateSolver for 1) = never
    int dm_factor = 0;
    int used_dm_factor = 0;  // the last synchronous call swept with the factor
    int dm_factor_rank = 0;  // the rank the last attempt found (0: rejected, or nothing was attempted)
    size_t timed_base = 0;   // timings a sweep keeps in front of its own (the factor kernels of the same call)
    int vxc_fringe = -1;  // k_vxc_ws at nao = 16 k + 1..4: whole-tile-row MFMA role with a vector fringe (1, -1 auto) or the padded grid (0)
    int used_vxc_fringe = 0; // what the last sweep's Vxc kernel was (DFT_GetOption "used_vxc_fringe")
    int used_publish = 0; // the last synchronous call was completed by 1: the stream write, 0: a kernel (DFT_GetOption "used_publish")
    int eri_sym = 0;   // 1: the caller vouches that the dense ERI is symmetric as an (N2, N2) matrix: DFT_ComputeCoulomb streams its upper
                       // triangle only; 2: ... and in each index pair, and dm = dm^T: the unique eighth only
    // A synchronous call seen before with the same pointers and sizes is replayed as one recorded HIP graph (one submission
    // instead of five launches): -1 auto = where the call is launch-bound (planes of at most GRAPH_AUTO_ELEMS doubles: H2O/def2-SVP
    // 30.4 -> 26.3 us per LDA call, 34.7 -> 32.9 GGA; Benzene/STO-3G 84.5 -> 86.0 and Benzene/def2-SVP 228.4 -> 230.6, so not there),
    // 1 always, 0 never.  An option change and any growth of the workspace drop the recorded graphs.
    int graph = -1;
    std::vector<SweepGraph> graphs;
    hipStream_t cap_stream = nullptr; // recording happens here (the caller's stream may be the null stream, which cannot record)
    unsigned long graph_clock = 0, graph_gen = 0;
    // workspace (`ws`: the planes of xc_sweep and of DFT_FxcPrepare / DFT_FxcApply, the set a recorded sweep holds)
    Planes ws;
    DevBuf dsym, slabs, exc, jpart, kpart, shells, msym, cdy, cdc, cdv, cdy2, cdc2, cdbt, ao_ws, vtmp, occ_cp, occ_dm, dmf_lt, dmf_c, dmf_st;
    int spin_wait = 1; // poll the host-mapped Exc instead of sleeping in hipStreamSynchronize
    int strict_sync = 0; // 1: after the Exc word, also poll the stream until it reports complete (+8-10 us per call)
    double *h_exc = nullptr;   // pinned, host-mapped: the reduce kernel writes Exc here
    double *h_exc_dev = nullptr; // device alias of h_exc
    // Completion without a kernel (option "publish"): the reduce kernel's finishing block stores Exc to h_exc itself, and the
    // word that says "the whole call has completed" is a per-call sequence number, written BEHIND that kernel by a stream
    // memory operation (hipStreamWriteValue64: performed after all earlier commands of the stream have completed).  The
    // synchronous call spins on the sequence word, then reads Exc.  Probed once at creation; where the runtime refuses the
    // operation on this allocation the one-thread k_publish_exc launch stays.
    int publish = -1;          // 0: k_publish_exc, 1: stream write (where the probe passed), -1 auto (= 1 where the probe passed)
    bool publish_ok = false;   // the probe's verdict
    unsigned long long *h_seq = nullptr, *h_seq_dev = nullptr; // pinned, host-mapped sequence word and its device alias
    unsigned long long seq = 0; // value of the last stream write that was enqueued
    bool recording = false;    // xc_sweep is being recorded into a graph: stream memory operations are not recorded
    int wait_mode = 0;         // how the last sweep with want_host_exc signals completion: 0 Exc word, 1 sequence word, 2 neither (synchronise)
    // Linear response of Vxc, one slot per kind: 0 the shipped formulas differentiated (DFT_FxcPrepare / DFT_FxcApply); 1 triplet,
    // 2 singlet through the spin-resolved bodies (DFT_FxcPrepareSpin).  Each has its own table and its own grad rho0, so that
    // prepares at different dm0 and applies of every kind interleave freely.
    FxcSlot fxc[3];
    // DFT_FxcPrepareSpinPol: the second-derivative table of the energy at (rho0_a, rho0_b) and the two ground-state gradients,
    // a slot of its own again; DFT_FxcApplySpinPol works in the planes of the synchronous entries below
    FxcSlot fxc_pol;
    // The synchronous entries past xc_sweep -- DFT_ComputeXCSpin, DFT_ComputeXCMeta, DFT_ComputeXCMetaSpin, DFT_ComputeTau,
    // DFT_ComputeTauSpin -- and the open-shell response pair (DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol) work in one set,
    // in stream order: the planes of each spin (a closed-shell call uses [0]; sigma, which nobody reads, and the Exc partials
    // with [0] alone), tau of each spin (2 ngrid), the tau coefficients (four planes per spin: ct_s and, for the plain form,
    // three of zeros), the padded matrix of each spin that k_tau reads (2 NP^2), the slabs of k_vxc_tau, the matrix one plain
    // contraction leaves, and the scalar of Exc.  An entry reserves what it uses at the size of its call, and every call
    // writes whole what it reads.  No recorded sweep and no prepared response table holds or reads any of them.
    Planes sync_ws[2];
    DevBuf sync_tau, sync_ct, sync_dp, sync_slabs, sync_vtmp, sync_exc;
    // The eight gradient-side entries -- DFT_ComputeXCGradient / Spin / Meta / MetaSpin and DFT_ComputeXCEnergyDensity / Spin / Meta /
    // MetaSpin -- work in
    // one set of their own, in stream order: the planes of each spin (a closed-shell call uses [0]; sigma and the Exc partials,
    // which nobody reads, with [0] alone), the padded matrix of each spin (NP^2 apart) that k_xc_grad and k_tau read -- every
    // entry symmetrises into it, none into the shared Dsym -- tau and its coefficient plane (meta entries; beta's ngrid after
    // alpha's), and the slabs of the
    // contraction (as many as the call's form writes).  An entry reserves what it uses at the size of its call, and every call
    // writes whole what it reads.  No recorded sweep and no prepared response table holds or reads any of them.
    Planes xcg[2];
    DevBuf xcg_dp, xcg_tau, xcg_ct, xcg_slabs;
    // DFT_ComputeXCGradientSpin.  1 (default): k_xc_grad on both spins' (coef, D) pairs in one launch (0.64 x / 0.82 x of the two
    // launches at 143 556 x 114 / 60 000 x 494, GGA: profiles/xc_gradient_spin_time.txt); 0: k_xc_grad once per spin into two slab
    // sets, what the tests hold the two-spin instantiation to
    int xcg_spin_fused = 1;
    // DFT_BeckeWeightGradient: [atoms (natm, 3) | a_CD (natm, natm) | 1 / R_CD (natm, natm)] on the device and the host copy they
    // were made from (uploaded again only when the atoms change), and the slabs of the kernel
    DevBuf becke_tab, becke_slabs;
    // The tau term of the potential.  0 (default): the sweep's contraction once per plane with the plane in the AO slot; 1:
    // k_vxc_tau, one pass over the three gradient planes.  The dedicated kernel does not beat the plain form (605.8 against 294.8 us
    // at 143 556 x 114, 2015.7 against 1855.1 us at 60 000 x 494: profiles/meta_time.txt), so it is the option, held to the plain
    // form by the tests
    int meta_fused = 0;
    // The tau stage of an open-shell call.  1 (default): k_tau_spin, one staging of the gradient rows for both spins
    // (xc_meta_spin.hip; 0.80 x / 0.61 x of the two launches at 143 556 x 114 / 60 000 x 494: profiles/meta_spin_time.txt); 0:
    // k_tau once per spin, what the tests hold the two-spin kernel to
    int tau_spin_fused = 1;
    // The contraction of DFT_ComputeXCGradientMeta.  1 (default): k_xc_grad_meta<true>, everything in one pass over the ten planes
    // (0.90 x / 0.80 x of the plain form at 143 556 x 114 / 60 000 x 494, TPSS: profiles/xc_gradient_meta_time.txt); 0: k_xc_grad on
    // c0..c3 and k_xc_grad_meta<false> (the tau term) into two slab sets and one sum, what the tests hold the fused kernel to
    int xcg_meta_fused = 1;
    // The contraction of DFT_ComputeXCGradientMetaSpin.  1 (default): k_xc_grad_meta_spin, both spins in one pass over the ten planes
    // (0.65 x / 0.59 x of the plain form at 143 556 x 114 / 60 000 x 494, TPSS: profiles/xc_gradient_meta_spin_time.txt); 0: per spin
    // k_xc_grad on c0..c3 and k_xc_grad_meta<false> (the tau term) into four slab sets and one sum, what the tests hold the fused
    // kernel to
    int xcg_meta_spin_fused = 1;
    std::vector<double> becke_tab_host;
    std::string last_error;
    std::vector<Timing> timings;
    size_t n_timed = 0;
    // AO shell-table cache key
    std::vector<unsigned char> shell_blob;
};

namespace {

void set_error(XCSolver *s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "libdft: %s\n", buf);
    if (s) s->last_error = buf;
}

bool hip_ok(XCSolver *s, hipError_t e, const char *what)
{
    if (e == hipSuccess) return true;
    set_error(s, "%s failed: %s", what, hipGetErrorString(e));
    return false;
}

void drop_graphs(XCSolver *s)
{
    for (SweepGraph &g : s->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    s->graphs.clear();
    ++s->graph_gen;
}

bool reserve(XCSolver *s, DevBuf &b, size_t bytes, const char *what, bool recorded = true)
{
    if (bytes <= b.cap) return true;
    if (recorded) drop_graphs(s); // recorded launches hold the old workspace pointers (false: a buffer no recorded sweep touches)
    if (b.p) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    if (!hip_ok(s, hipMalloc(&b.p, want), what)) return false;
    b.cap = want;
    return true;
}

// rho of `ngrid` points, and of the rest what the entry uses: the coefficient planes, grad rho and sigma (the last two for a
// gradient-corrected functional only), `nxb` Exc partials.  `recorded`: the set is `ws`, which recorded sweeps hold.
enum : unsigned { WS_COEF = 1, WS_GRAD = 2, WS_SIGMA = 4, WS_ALL = 7 };

bool reserve_planes(XCSolver *s, Planes &w, bool recorded, long ngrid, unsigned parts, long nxb = 0)
{
    const size_t ng = sizeof(double) * (size_t)ngrid;
    const bool gga = s->needs_grad;
    return reserve(s, w.rho, ng, "hipMalloc(rho)", recorded) &&
           (!(parts & WS_COEF) || reserve(s, w.coef, ng * (gga ? 4 : 1), "hipMalloc(coef)", recorded)) &&
           (!nxb || reserve(s, w.partial, sizeof(double) * nxb, "hipMalloc(partial)", recorded)) &&
           (!(gga && (parts & WS_SIGMA)) || reserve(s, w.sigma, ng, "hipMalloc(sigma)", recorded)) &&
           (!(gga && (parts & WS_GRAD)) || reserve(s, w.grad, 3 * ng, "hipMalloc(grad)", recorded));
}

// 0 LDA, 1 GGA, 2 B3LYP, 3 mix: what the launchers in the other translation units take for the solver's type
int xc_type_index(const XCSolver *s)
{
    return s->type == SOLVER_LDA ? 0 : s->type == SOLVER_GGA ? 1 : s->type == SOLVER_B3LYP ? 2 : 3;
}

// What every XC entry does first, in two halves: the solver's kind, then the device, the sizes and ao_grad.  `timed`: timings of
// the same call that stay in front of the entry's own.  `meta_who`: the name of an entry that forms tau (null: any other).
// enter_sizes is itself two steps, which the gradient-side entries (xcg_enter) take apart: they name every fault of the
// arguments before the device.
bool enter_kind(XCSolver *s, size_t timed = 0, const char *meta_who = nullptr)
{
    s->last_error.clear();
    s->n_timed = timed;
    if (meta_who && !s->is_meta) {
        set_error(s, "%s needs a solver made by DFT_CreateSolverMeta (this one carries no meta-GGA weights)", meta_who);
        return false;
    }
    if (s->meta_active && !meta_who) {
        set_error(s, "the solver's functional is a meta-GGA (non-zero tpss_x / tpss_c weight): it reads the kinetic-energy density, "
                     "which only DFT_ComputeXCMeta and DFT_ComputeXCMetaSpin form; this entry would drop it");
        return false;
    }
    return true;
}

bool device_ready(XCSolver *s)
{
    if (!s->device_ok) set_error(s, "no usable HIP device");
    return s->device_ok;
}

bool sizes_ok(XCSolver *s, long ngrid, int nao, const double *ao_grad)
{
    if (ngrid <= 0 || nao <= 0) {
        set_error(s, "bad sizes ngrid=%ld nao=%d", ngrid, nao);
        return false;
    }
    if (s->needs_grad && !ao_grad) {
        set_error(s, "ao_grad pointer is null for a gradient-corrected functional");
        return false;
    }
    return true;
}

bool enter_sizes(XCSolver *s, long ngrid, int nao, const double *ao_grad)
{
    return device_ready(s) && sizes_ok(s, ngrid, nao, ao_grad);
}

bool enter(XCSolver *s, long ngrid, int nao, const double *ao_grad, size_t timed = 0)
{
    return enter_kind(s, timed) && enter_sizes(s, ngrid, nao, ao_grad);
}

// Every entry point runs on the solver's device (its workspace and stream live there): a caller that
// switched devices since DFT_CreateSolver gets the solver's device for the call and its own back after.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const XCSolver *s)
    {
        if (!s || !s->device_ok) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != s->device) switched = hipSetDevice(s->device) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

struct ScopedTimer {
    XCSolver *s;
    size_t idx = 0;
    bool on;
    ScopedTimer(XCSolver *s_, const char *name) : s(s_), on(s_->profile != 0)
    {
        if (!on) return;
        idx = s->n_timed++;
        if (idx >= s->timings.size()) {
            Timing t{name, nullptr, nullptr};
            (void)hipEventCreate(&t.t0);
            (void)hipEventCreate(&t.t1);
            s->timings.push_back(t);
        }
        s->timings[idx].name = name;
        (void)hipEventRecord(s->timings[idx].t0, s->stream);
    }
    ~ScopedTimer()
    {
        if (on) (void)hipEventRecord(s->timings[idx].t1, s->stream);
    }
};

int auto_ksplit(const XCSolver *s, long ngrid, int nblk)
{
    if (s->ksplit > 0) return s->ksplit;
    // enough workgroups to fill the chip a few times over, >= 256 points each
    long want = (4L * s->num_cu + nblk - 1) / nblk;
    long maxsplit = (ngrid + 255) / 256;
    if (want > maxsplit) want = maxsplit;
    if (want < 1) want = 1;
    return (int)want;
}

// Runtime values to template arguments, for kernel launches written once as generic lambdas:
// f(std::integral_constant<int, NT>) for a tile count nt = 1..8, f(std::true_type / std::false_type) for a bool.
template <int NT = 1, class F>
void with_nt(int nt, F &&f)
{
    if constexpr (NT < 8) {
        if (nt != NT) return with_nt<NT + 1>(nt, f);
    }
    f(std::integral_constant<int, NT>{});
}

template <class F>
void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else   f(std::false_type{});
}

// Small bases: the whole sweep in one kernel (planes below 4 GiB: one buffer descriptor each)
bool takes_tiny(const XCSolver *s, long ngrid, int nao)
{
    return s->path == 0 && s->tiny != 0 && s->type != SOLVER_MIX && nao <= TINY_MAX_NAO && (double)ngrid * nao * 8.0 < 4294967296.0 &&
           (s->tiny > 0 || tiny_pays(s->num_cu, xc_type_index(s), nao, ngrid));
}

// How a sweep over (ngrid, nao) planes is cut up: which kernel family, how many slabs, the chunk of a split-K launch.
// Shared by the ground-state sweep and the response entries (DFT_FxcPrepare / DFT_FxcApply), which must choose alike.
struct SweepPlan {
    int NP = 0, nblk = 0, ntv = 0, nslab = 0, nA = 0, nB = 0, npair = 0;
    long chunk = 0;
    bool gga = false, fits32 = false, fast = false, big = false, vec16 = false;
    const double *gx = nullptr, *gy = nullptr, *gz = nullptr;
};

SweepPlan plan_sweep(const XCSolver *s, long ngrid, int nao, const double *ao, const double *ao_grad, bool tiny)
{
    const bool gga = s->needs_grad;
    const int NP = ((nao + 15) / 16) * 16;
    const int nblk = (nao + 127) / 128;
    // the wave-specialised kernels address a plane through ONE buffer descriptor: planes of 4 GiB or more
    // (ngrid*nao >= 2^29) take the generic tiled kernels
    const bool fits32 = (double)ngrid * nao * 8.0 < 4294967296.0;
    const bool fast = s->path == 0 && nao <= 128 && fits32;
    const bool big = s->path == 0 && nao > 128;   // nao <= 128 with planes >= 4 GiB: the generic MFMA kernels below
    const int ntv = NP / 16;
    int nslab;
    long chunk = 0;
    const int nA = (nao + BG_BM - 1) / BG_BM, nB = (nao + BG_BN - 1) / BG_BN, npair = nA * nB;
    if (big) {
        // split-K over grid chunks; chunks are dealt to XCDs (blockIdx % 8), so ksplit is a multiple of 8
        // chunks per XCD: the candidate (<= 32, slabs <= 2 GB, >= 64 grid rows per chunk) whose workgroup
        // count fills whole waves of the chip best (360 workgroups on 256 CUs lost 30 % to the tail)
        long per_xcd = 1;
        double best = 0.0;
        for (long c = 1; c <= 32; ++c) {
            const long wgs = 8L * npair * c;
            if (8 * c * 64 > ngrid && c > 1) break;
            if ((double)(8 * c) * nao * nao * 8.0 > 2.0e9 && c > 1) break;
            const long rounds = (wgs + s->num_cu - 1) / s->num_cu;
            const double eff = (double)wgs / (double)(rounds * s->num_cu);
            if (eff > best + 1e-9) { best = eff; per_xcd = c; }
        }
        // a chunk of one plane stays below 4 GiB: k_vxc_big addresses it through one buffer descriptor
        while ((double)((ngrid + 8 * per_xcd - 1) / (8 * per_xcd) + BG_BK) * nao * 8.0 >= 4294967296.0) ++per_xcd;
        nslab = (int)(8 * per_xcd);
        chunk = (ngrid + nslab - 1) / nslab;
        chunk = ((chunk + BG_BK - 1) / BG_BK) * BG_BK;
    } else if (tiny) {
        nslab = tiny_workgroups(s->num_cu, xc_type_index(s), nao, ngrid);   // (a mix never takes this kernel)
    } else if (fast) {
        const long ntile = (ngrid + WS_ROWS - 1) / WS_ROWS;
        nslab = (int)std::min<long>(s->num_cu, ntile); // one persistent, wave-specialised workgroup per CU
    } else {
        const int nsplit = auto_ksplit(s, ngrid, nblk * nblk);
        chunk = (ngrid + nsplit - 1) / nsplit;
        chunk = ((chunk + 31) / 32) * 32;
        nslab = (int)((ngrid + chunk - 1) / chunk);
    }
    SweepPlan P;
    P.NP = NP; P.nblk = nblk; P.ntv = ntv; P.nslab = nslab; P.nA = nA; P.nB = nB; P.npair = npair;
    P.chunk = chunk;
    P.gga = gga; P.fits32 = fits32; P.fast = fast; P.big = big;
    const size_t ng = (size_t)ngrid;
    P.gx = ao_grad; P.gy = gga ? ao_grad + ng * nao : nullptr; P.gz = gga ? ao_grad + 2 * ng * nao : nullptr;
    // 16-byte plane loads: even nao and every plane 16-byte aligned
    P.vec16 = (nao % 2 == 0) && ((((uintptr_t)ao | (uintptr_t)P.gx | (uintptr_t)P.gy | (uintptr_t)P.gz) & 15) == 0);
    return P;
}

// Density step through the matrix: rho, grad rho (interleaved, 3 per point) and sigma of ANY dm (the kernels see its
// symmetric part).  Linear in dm, so the same launches give rho1 / grad rho1 of a perturbation.
void launch_density(XCSolver *s, const SweepPlan &P, long ngrid, int nao, const double *dm, const double *ao, double *Dp,
                    double *rho, double *grad, double *sigma)
{
    const int NP = P.NP, ntv = P.ntv, nslab = P.nslab;
    const bool gga = P.gga, fast = P.fast, big = P.big, vec16 = P.vec16;
    const double *gx = P.gx, *gy = P.gy, *gz = P.gz;
    hipStream_t st = s->stream;
    if (!fast) { // the wave-specialised rho kernel symmetrises D in its prologue
        ScopedTimer t(s, "sym_dm");
        dim3 b(16, 16), g(NP / 16, NP / 16);
        hipLaunchKernelGGL(k_sym_dm, g, b, 0, st, nao, NP, dm, Dp);
    }
    {
        ScopedTimer t(s, "rho");
        with_bool(gga, [&](auto G) {
            if (fast)
                with_bool(vec16, [&](auto V) { with_nt(ntv, [&](auto NT) {
                    hipLaunchKernelGGL((k_rho_ws<NT, G, V>), dim3((unsigned)nslab), dim3(WS_THREADS), 0, st, ngrid, nao, ao, gx, gy, gz, dm, rho, grad, sigma, s->sweep_order & 1);
                }); });
            else if (big) // 64-row workgroups, two per CU
                with_bool(vec16, [&](auto V) {
                    hipLaunchKernelGGL((k_rho_big64<G, V>), dim3((unsigned)((ngrid + R6_BM - 1) / R6_BM)), dim3(256), 0, st, ngrid, nao, NP, ao, gx, gy, gz, Dp, rho, grad, sigma);
                });
            else if (s->path != 1)
                hipLaunchKernelGGL(k_rho_mfma<G>, dim3((unsigned)((ngrid + 63) / 64)), dim3(256), 0, st, ngrid, nao, NP, ao, gx, gy, gz, Dp, rho, grad, sigma);
            else
                hipLaunchKernelGGL(k_rho_valu<G>, dim3((unsigned)((ngrid + 3) / 4)), dim3(256), 0, st, ngrid, nao, NP, ao, gx, gy, gz, Dp, rho, grad, sigma);
        });
    }
}

// Contraction of the coefficient planes with the AO planes into slabs, and the slab reduce into V (for B3LYP: M + M^T).
// `fin` non-null (the ground-state sweep): the reduce also finishes Exc from the partials, as the options say; null (the
// response of Vxc, DFT_FxcApply): the same kernels, no energy, no publishing, nothing for the host to wait on.
struct ExcFinish {
    long nxb;
    const double *partial;
    double *exc;
    bool want_host_exc;
};

bool vxc_stage(XCSolver *s, const SweepPlan &P, bool tiny, long ngrid, int nao, const double *ao, const double *coef,
               double *slabs, double *vxc, const ExcFinish *fin)
{
    const int nblk = P.nblk, ntv = P.ntv, nslab = P.nslab, nB = P.nB, npair = P.npair;
    const long chunk = P.chunk;
    const bool gga = P.gga, fast = P.fast, big = P.big, vec16 = P.vec16;
    const double *gx = P.gx, *gy = P.gy, *gz = P.gz;
    const long nxb = fin ? fin->nxb : 0;
    const double *partial = fin ? fin->partial : nullptr;
    double *exc = fin ? fin->exc : nullptr;
    const bool want_host_exc = fin && fin->want_host_exc;
    hipStream_t st = s->stream;
    if (!tiny) {
        ScopedTimer t(s, fin ? "vxc" : "fxc_vxc");
        // Option "vxc_fringe": at nao = 16 k + 1..4 (k >= 1) the one-sided kernels leave the k x k whole tiles to the matrix
        // pipe and take the fringe lines on the vector ALU (vxc_ws_mfma_fringe) instead of padding to k + 1 tiles per side
        const bool fringe = fast && s->type != SOLVER_B3LYP && s->vxc_fringe != 0 && nao > 16 && nao % 16 >= 1 && nao % 16 <= 4;
        s->used_vxc_fringe = fringe;
        auto launch = [&](auto G, auto S) { // S: B3LYP, the wave-specialised kernels write symmetrised slabs
            if (fast)
                with_bool(vec16, [&](auto V) { with_nt(ntv, [&](auto NT) {
                    if constexpr (NT >= 2 && !S) {
                        if (fringe) {
                            hipLaunchKernelGGL((k_vxc_ws<NT, G, V, false, true>), dim3((unsigned)nslab), dim3(WS_THREADS), 0, st, ngrid, nao, ao, gx, gy, gz, coef, slabs, (s->sweep_order >> 1) & 1);
                            return;
                        }
                    }
                    hipLaunchKernelGGL((k_vxc_ws<NT, G, V, S>), dim3((unsigned)nslab), dim3(WS_THREADS), 0, st, ngrid, nao, ao, gx, gy, gz, coef, slabs, (s->sweep_order >> 1) & 1);
                }); });
            else if (big)
                with_bool(vec16, [&](auto V) {
                    hipLaunchKernelGGL((k_vxc_big<G, V>), dim3((unsigned)(nslab * npair)), dim3(BG_THREADS), 0, st, ngrid, nao, chunk, nB, npair, ao, gx, gy, gz, coef, slabs);
                });
            else if (s->path != 1)
                hipLaunchKernelGGL(k_vxc_mfma<G>, dim3((unsigned)nslab, nblk, nblk), dim3(256), 0, st, ngrid, nao, chunk, ao, gx, gy, gz, coef, slabs);
            else
                hipLaunchKernelGGL(k_vxc_valu<G>, dim3((unsigned)nslab), dim3(256), 0, st, ngrid, nao, chunk, ao, gx, gy, gz, coef, slabs);
        };
        switch (s->type) { // (G, S)
        case SOLVER_LDA: launch(std::false_type{}, std::false_type{}); break;
        case SOLVER_GGA: launch(std::true_type{}, std::false_type{}); break;
        case SOLVER_MIX: // GGA convention: one-sided, never symmetrised here; an LDA-class mix takes the one-plane kernels
            if (gga) launch(std::true_type{}, std::false_type{});
            else     launch(std::false_type{}, std::false_type{});
            break;
        default:         launch(std::true_type{}, std::true_type{}); break;
        }
    }
    {
        ScopedTimer t(s, fin ? "reduce_vxc" : "fxc_reduce");
        dim3 g((unsigned)(((size_t)nao * nao + 31) / 32));
        const bool b3 = s->type == SOLVER_B3LYP;
        if (b3 && big) { // plain reduce into M, then tiled M + M^T
            if (!reserve(s, s->msym, sizeof(double) * (size_t)nao * nao, "hipMalloc(M)")) return false;
            double *M = (double *)s->msym.p;
            hipLaunchKernelGGL(k_reduce_slabs8<false>, g, dim3(256), 0, st, nao, nslab, slabs, M);
            const int nt = (nao + 31) / 32;
            hipLaunchKernelGGL(k_symmetrize, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, nao, M, vxc);
        } else if (b3 && !fast) {
            hipLaunchKernelGGL(k_reduce_slabs8<true>, g, dim3(256), 0, st, nao, nslab, slabs, vxc);
        } else if (!fin) { // the response of Vxc: no energy to finish (wave-specialised slabs are already symmetrised for B3LYP)
            hipLaunchKernelGGL(k_reduce_slabs8<false>, g, dim3(256), 0, st, nao, nslab, slabs, vxc);
        } else if (s->fuse_finish) { // wave-specialised slabs are already symmetrised for B3LYP
            // last launch of the call: its last-ticket block also finishes Exc (device scalar + host-mapped word)
            hipLaunchKernelGGL((k_reduce_slabs8<false, true>), g, dim3(256), 0, st, nao, nslab, slabs, vxc, nxb, partial, exc,
                               want_host_exc ? s->h_exc_dev : nullptr);
            return hip_ok(s, hipGetLastError(), "XC sweep launch");
        } else {
            // Exc is summed by the reduce kernel's highest-index block into the DEVICE scalar only; publishing it to the host
            // is left to a one-thread kernel behind it (stream order: the whole call has completed when the word appears) --
            // the shortest launch there is, instead of a finishing kernel that still has the partials to add up
            // Option "publish" (where the creation-time probe passed): no publishing launch -- the reduce kernel's finishing
            // block stores Exc to the host word, and a stream memory write behind the kernel raises the sequence word the
            // host waits for.  Same meaning (stream order: after every store of the call), no dispatch.
            const bool sw = want_host_exc && s->h_exc_dev && s->publish > 0 && s->publish_ok && !s->recording;
            hipLaunchKernelGGL((k_reduce_slabs8<false, true>), g, dim3(256), 0, st, nao, nslab, slabs, vxc, nxb, partial, exc,
                               sw ? s->h_exc_dev : (double *)nullptr);
            if (sw) {
                if (hipStreamWriteValue64(st, s->h_seq_dev, s->seq + 1, 0) == hipSuccess) {
                    ++s->seq;
                    s->wait_mode = 1;
                } else { // refused after all: this call is waited for on the stream, later ones publish by kernel
                    (void)hipGetLastError();
                    s->publish_ok = false;
                    s->wait_mode = 2;
                }
            } else if (want_host_exc && s->h_exc_dev) {
                hipLaunchKernelGGL(k_publish_exc, dim3(1), dim3(1), 0, st, exc, s->h_exc_dev);
            }
            return hip_ok(s, hipGetLastError(), "XC sweep launch");
        }
        // last launch of the call: Exc to the device scalar and to host-mapped memory
        if (fin) hipLaunchKernelGGL(k_finish_exc, dim3(1), dim3(256), 0, st, nxb, partial, exc, want_host_exc ? s->h_exc_dev : nullptr);
    }
    return hip_ok(s, hipGetLastError(), "XC sweep launch");
}

// The buffers every entry shares, in stream order: the padded, symmetrised matrix and the contraction's slabs
bool reserve_dsym(XCSolver *s, const SweepPlan &P)
{
    return reserve(s, s->dsym, sizeof(double) * P.NP * P.NP, "hipMalloc(Dsym)");
}

bool reserve_slabs(XCSolver *s, const SweepPlan &P, int nao)
{
    return reserve(s, s->slabs, sizeof(double) * (size_t)P.nslab * nao * nao, "hipMalloc(slabs)");
}

// Occupied-orbital density step: 16 nch nocc_tiles MFMAs per 16 grid rows (8 for LDA) against 4 NT^2 through the
// full matrix; taken when it does clearly fewer (the two kernels run at similar matrix-pipe efficiency), on the
// production path only.
bool occ_allowed(const XCSolver *s)
{
    return s->path == 0 && s->occ != 2;
}

bool occ_pays(const XCSolver *s, int nao, int nocc, OccPlan &plan)
{
    if (!occ_allowed(s)) return false;
    plan = occ_plan(nao, nocc, s->needs_grad);
    return s->occ == 1 || plan.mfma_occ <= 0.85 * plan.mfma_full;
}

// Where a call's density comes from, decided once (density_source) and run by run_density: the occupied-orbital kernels
// on `cocc` (nao, nocc) with dm = cocc cocc^T, or the matrix kernels on `dm` -- the caller's, or built from cocc first.
struct DensitySource {
    bool use_occ = false;
    OccPlan oplan;
    const double *dm = nullptr, *cocc = nullptr;
    int nocc = 0;
};

// `may_occ` false: the entry's plan has no occupied-orbital form (the one-kernel sweep for small bases)
bool density_source(XCSolver *s, int nao, const double *dm, const double *cocc, int nocc, bool may_occ, DensitySource &d)
{
    if (!dm && !cocc) {
        set_error(s, "neither a density matrix nor occupied orbitals were given");
        return false;
    }
    if (cocc && nocc <= 0) {
        set_error(s, "occupied orbitals given with nocc=%d", nocc);
        return false;
    }
    d.use_occ = cocc && may_occ && occ_pays(s, nao, nocc, d.oplan);
    s->used_occ = d.use_occ;
    if (!d.use_occ && !dm) { // the dm kernels need the matrix itself
        if (!reserve(s, s->occ_dm, sizeof(double) * (size_t)nao * nao, "hipMalloc(dm)")) return false;
        launch_dm_from_cocc(s->stream, nao, nocc, cocc, s->occ_dm.d());
        dm = s->occ_dm.d();
    }
    d.dm = dm;
    d.cocc = cocc;
    d.nocc = nocc;
    return true;
}

bool run_density(XCSolver *s, const SweepPlan &P, const DensitySource &d, long ngrid, int nao, const double *ao, double *rho,
                 double *grad, double *sigma)
{
    if (!d.use_occ) {
        launch_density(s, P, ngrid, nao, d.dm, ao, s->dsym.d(), rho, grad, sigma);
        return true;
    }
    ScopedTimer t(s, "rho_occ");
    if (!reserve(s, s->occ_cp, sizeof(double) * d.oplan.cp_doubles, "hipMalloc(packed cocc)")) return false;
    return hip_ok(s, launch_rho_occ(s->stream, s->num_cu, d.oplan, P.gga, P.vec16, ngrid, nao, d.nocc, d.cocc, s->occ_cp.d(), ao, P.gx, P.gy,
                                    P.gz, rho, grad, sigma), "occupied-orbital density launch");
}

// The functional at the points of `p`'s density: coefficient planes for the contraction and one Exc partial per workgroup
void launch_xc_points(XCSolver *s, long ngrid, long nxb, const double *w, const Planes &p)
{
    ScopedTimer t(s, "xc_points");
    const dim3 g((unsigned)nxb), b(256);
    hipStream_t st = s->stream;
    double *rho = p.rho.d(), *sigma = p.sigma.d(), *grad = p.grad.d(), *coef = p.coef.d(), *partial = p.partial.d();
    switch (xc_type_index(s)) {
    case 0: hipLaunchKernelGGL(k_xc_points<0>, g, b, 0, st, ngrid, rho, sigma, grad, w, coef, partial, s->quirks); break;
    case 1: hipLaunchKernelGGL(k_xc_points<1>, g, b, 0, st, ngrid, rho, sigma, grad, w, coef, partial, s->quirks); break;
    case 2: hipLaunchKernelGGL(k_xc_points<2>, g, b, 0, st, ngrid, rho, sigma, grad, w, coef, partial, s->quirks); break;
    default:
        with_bool(s->needs_grad, [&](auto G) {
            hipLaunchKernelGGL(k_xc_points_mix<G>, g, b, 0, st, ngrid, rho, sigma, grad, w, coef, partial, s->quirks, s->mix);
        });
    }
}

// The sweep: everything on s->stream, Exc left in s->exc (device).
// `cocc` (nao, nocc) with dm = cocc cocc^T switches the density step to the occupied-orbital form where that
// pays (xc_occ_kernels.hpp); `dm` may then be null.
bool xc_sweep(XCSolver *s, long ngrid, int nao, const double *dm, const double *ao,
              const double *ao_grad, const double *w, double *vxc, bool want_host_exc,
              const double *cocc = nullptr, int nocc = 0, double *exc_out = nullptr)
{
    const size_t timed = s->timed_base;   // non-zero only for the sweep of a call that factorised its dm first
    s->timed_base = 0;
    s->wait_mode = 0;
    s->used_vxc_fringe = 0;
    if (!enter(s, ngrid, nao, ao_grad, timed)) return false;
    const bool tiny = takes_tiny(s, ngrid, nao);
    DensitySource src;
    if (!density_source(s, nao, dm, cocc, nocc, !tiny, src)) return false;
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, tiny);
    const long nxb = tiny ? P.nslab : (ngrid + 255) / 256; // Exc partials: one per workgroup of the kernel that evaluates the functional
    if (!reserve_dsym(s, P) || !reserve_planes(s, s->ws, true, ngrid, WS_ALL, nxb) || !reserve_slabs(s, P, nao) ||
        !reserve(s, s->exc, 2 * sizeof(double), "hipMalloc(exc)"))   // the device-side Exc scalar
        return false;
    const Planes &p = s->ws;
    double *exc = exc_out ? exc_out : s->exc.d();   // the asynchronous entries' caller-owned scalar: written by the finishing kernel itself
    if (tiny) {
        ScopedTimer t(s, "sweep_tiny");
        launch_sweep_tiny(s->stream, P.nslab, xc_type_index(s), ngrid, nao, ao, P.gx, P.gy, P.gz, src.dm, w, s->slabs.d(), p.partial.d(),
                          s->quirks);
    } else {
        if (!run_density(s, P, src, ngrid, nao, ao, p.rho.d(), p.grad.d(), p.sigma.d())) return false;
        launch_xc_points(s, ngrid, nxb, w, p);
    }
    const ExcFinish fin{nxb, p.partial.d(), exc, want_host_exc};
    return vxc_stage(s, P, tiny, ngrid, nao, ao, p.coef.d(), s->slabs.d(), vxc, &fin);
}

// The refusal DFT_ComputeXCSpin and the open-shell response share: second and first derivatives of the ENERGY.
bool spin_quirks_ok(XCSolver *s, const char *who)
{
    const int type = xc_type_index(s);
    if (s->quirks && (type == 0 || type == 1 || (type == 3 && (s->mix.c[XC_VWN5_C] != 0.0 || s->mix.c[XC_PBE_C] != 0.0)))) {
        set_error(s, "%s: the spin-resolved potentials are the first derivatives of the energy, but with quirks = 1 the "
                     "ground state solved the shipped vwn5_c / pbe_c potentials, which are not the derivatives of their energies; "
                     "run with --quirks 0", who);
        return false;
    }
    return true;
}

// The density kernels on the matrix of spin alpha, then of spin beta (linear in the matrix), into the planes of the
// synchronous entries; `ga`, `gb`: where the two gradients go.  sigma is what the kernels write beside the gradient; nobody
// reads it.
void launch_density_spin(XCSolver *s, const SweepPlan &P, long ngrid, int nao, const double *dm_a, const double *dm_b, const double *ao,
                         double *ga, double *gb)
{
    double *sigma = s->sync_ws[0].sigma.d(), *Dp = s->dsym.d();
    launch_density(s, P, ngrid, nao, dm_a, ao, Dp, s->sync_ws[0].rho.d(), ga, sigma);
    launch_density(s, P, ngrid, nao, dm_b, ao, Dp, s->sync_ws[1].rho.d(), gb, sigma);
}

// The launches of a tau stage on `nspin` matrices that are already padded and symmetrised (Dp, NP^2 apart).  `both`: the plan is
// tau_spin_plan's and k_tau_spin takes the two matrices at once (anything but two is refused here); otherwise the plan is
// tau_plan's and k_tau runs once per spin.
bool launch_tau_stage(XCSolver *s, const TauPlan &tp, bool both, int nspin, long ngrid, int nao, const double *ao_grad, const double *Dp,
                      double *const tau[2])
{
    static const char *const what[2][2] = {{"tau launch", "tau launch"}, {"tau launch (alpha)", "tau launch (beta)"}};
    const size_t np2 = (size_t)tp.NP * tp.NP;
    if (nspin < 1 || nspin > 2 || (both && nspin != 2)) {
        set_error(s, "tau stage: %s on %d matrices", both ? "the two-spin kernel" : "the one-spin kernel", nspin);
        return false;
    }
    if (both) return hip_ok(s, launch_tau_spin(s->stream, tp, ngrid, nao, ao_grad, Dp, Dp + np2, tau[0], tau[1]), "two-spin tau launch");
    for (int sp = 0; sp < nspin; ++sp)
        if (!hip_ok(s, launch_tau(s->stream, tp, ngrid, nao, ao_grad, Dp + sp * np2, tau[sp]), what[nspin - 1][sp])) return false;
    return true;
}

// tau of one spin or of both (DFT_ComputeTau, DFT_ComputeTauSpin and the meta-GGA sweeps): the padded symmetric matrix of each
// spin into the entries' buffer, then k_tau_spin (two spins with option "tau_spin_fused" = 1) or k_tau once per spin.
bool compute_tau(XCSolver *s, int nspin, long ngrid, int nao, const double *const dm[2], const double *ao_grad, double *const tau[2])
{
    const bool both = nspin == 2 && s->tau_spin_fused;
    const TauPlan tp = both ? tau_spin_plan(s->num_cu, ngrid, nao) : tau_plan(s->num_cu, ngrid, nao);
    const size_t np2 = (size_t)tp.NP * tp.NP;
    if (!reserve(s, s->sync_dp, sizeof(double) * nspin * np2, nspin == 2 ? "hipMalloc(meta Dp of both spins)" : "hipMalloc(meta Dp)", false)) return false;
    double *Dp = s->sync_dp.d();
    ScopedTimer t(s, nspin == 1 ? "tau" : both ? "tau_spin" : "tau x2");
    for (int sp = 0; sp < nspin; ++sp)
        hipLaunchKernelGGL(k_sym_dm, dim3(tp.NP / 16, tp.NP / 16), dim3(16, 16), 0, s->stream, nao, tp.NP, dm[sp], Dp + sp * np2);
    return launch_tau_stage(s, tp, both, nspin, ngrid, nao, ao_grad, Dp, tau);
}

// What tells DFT_ComputeXCSpin, DFT_ComputeXCMeta and DFT_ComputeXCMetaSpin apart: the entry's name, its sentence for a null
// pointer, the sweep's name in the NaN message, what a failed allocation of the Exc scalar and a failed pointwise launch are
// called, the number of spins, whether it forms tau, and whether ao_grad is among the pointers of `needs` (otherwise
// enter_sizes names it, for a gradient-corrected functional).
struct SyncEntry {
    const char *who, *needs, *what, *alloc_exc, *launch_points;
    int nspin;
    bool meta, grad_in_needs;
};

// The synchronous sweep of the three entries above, each stage once over sp < nspin: the closed-shell sweep's density kernels on
// each spin's matrix, tau (meta entries; zeros when both meta weights are), one pointwise kernel (xc_spin.hip, xc_meta.hip
// or xc_meta_spin.hip), the closed-shell contraction and reduce of each spin's coefficient planes -- the last reduce finishes
// Exc from the pointwise kernel's partials, as xc_sweep's does -- and the tau term of each spin added to its V in either form
// of "meta_fused".  Never the one-kernel plan for small bases (it keeps no density), never recorded.  Shares Dsym, the slabs
// and M with the other entries (stream order) and works in the planes of the synchronous entries otherwise: the response
// tables and the workspace a recorded sweep holds are not written.  Refusals, in this order for every entry: the solver's
// kind, a null pointer, then the device, the sizes and ao_grad (enter_sizes), then quirks = 1 -- all before anything touches
// the device, so that the first two can be told apart from "no usable HIP device".
bool xc_sweep_sync(XCSolver *s, const SyncEntry &E, long ngrid, int nao, const double *const dm[2], const double *ao, const double *ao_grad,
                   const double *w, double *const vxc[2], double *exc_host)
{
    const int nspin = E.nspin;
    if (!enter_kind(s, 0, E.meta ? E.who : nullptr)) return false;
    bool ptrs = ao && w && exc_host && (ao_grad || !E.grad_in_needs);
    for (int sp = 0; sp < nspin; ++sp) ptrs = ptrs && dm[sp] && vxc[sp];
    if (!ptrs) {
        set_error(s, "%s", E.needs);
        return false;
    }
    if (!enter_sizes(s, ngrid, nao, ao_grad) || !spin_quirks_ok(s, E.who)) return false;
    const bool gga = s->needs_grad, tau_term = E.meta && s->meta_active;
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, false);
    const long nxb = E.meta ? meta_points_blocks(ngrid) : spin_points_blocks(ngrid);
    const size_t ng = (size_t)ngrid, nn = (size_t)nao * nao;
    Planes *p = s->sync_ws;
    if (!reserve_dsym(s, P) || !reserve_slabs(s, P, nao) || !reserve_planes(s, p[0], false, ngrid, WS_ALL, nxb) ||
        (nspin == 2 && !reserve_planes(s, p[1], false, ngrid, WS_COEF | WS_GRAD)) ||
        (E.meta && (!reserve(s, s->sync_tau, sizeof(double) * nspin * ng, nspin == 2 ? "hipMalloc(tau of both spins)" : "hipMalloc(tau)", false) ||
                    !reserve(s, s->sync_ct, sizeof(double) * 4 * nspin * ng,
                             nspin == 2 ? "hipMalloc(tau coefficients of both spins)" : "hipMalloc(tau coefficient)", false))) ||
        !reserve(s, s->sync_exc, 2 * sizeof(double), E.alloc_exc, false))
        return false;
    for (int sp = 0; sp < nspin; ++sp)
        launch_density(s, P, ngrid, nao, dm[sp], ao, s->dsym.d(), p[sp].rho.d(), p[sp].grad.d(), p[0].sigma.d());
    double *ct = s->sync_ct.d();
    double *const tau[2] = {s->sync_tau.d(), E.meta ? s->sync_tau.d() + ng : nullptr};
    if (tau_term) {
        if (!compute_tau(s, nspin, ngrid, nao, dm, ao_grad, tau)) return false;
    } else if (E.meta && !hip_ok(s, hipMemsetAsync(tau[0], 0, sizeof(double) * nspin * ng, s->stream), "clear tau")) {
        return false;
    }
    {   // the one stage that differs in more than its loop count: three kernels
        ScopedTimer t(s, !E.meta ? "xc_points_spin" : nspin == 2 ? "xc_points_meta_spin" : "xc_points_meta");
        const hipError_t e =
            !E.meta ? launch_xc_points_spin(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, p[0].rho.d(), p[1].rho.d(), gga ? p[0].grad.d() : nullptr,
                                            gga ? p[1].grad.d() : nullptr, w, p[0].coef.d(), p[1].coef.d(), p[0].partial.d())
            : nspin == 2 ? launch_xc_points_meta_spin(s->stream, s->mix.c, s->meta, ngrid, p[0].rho.d(), p[1].rho.d(), p[0].grad.d(), p[1].grad.d(),
                                                      tau[0], tau[1], w, p[0].coef.d(), p[1].coef.d(), ct, ct + 4 * ng, p[0].partial.d())
                         : launch_xc_points_meta(s->stream, s->mix.c, s->meta, ngrid, p[0].rho.d(), p[0].grad.d(), tau[0], w, p[0].coef.d(), ct,
                                                 p[0].partial.d());
        if (!hip_ok(s, e, E.launch_points)) return false;
    }
    double *exc = s->sync_exc.d();
    const ExcFinish fin{nxb, p[0].partial.d(), exc, false};   // no host-mapped word, no publishing: Exc is copied below
    for (int sp = 0; sp < nspin; ++sp)
        if (!vxc_stage(s, P, false, ngrid, nao, ao, p[sp].coef.d(), s->slabs.d(), vxc[sp], sp == nspin - 1 ? &fin : nullptr)) return false;
    if (tau_term && s->meta_fused) {
        const VxcTauPlan vp = vxc_tau_plan(s->num_cu, ngrid, nao);
        if (!reserve(s, s->sync_slabs, sizeof(double) * (size_t)vp.nslab * nn, "hipMalloc(tau slabs)", false)) return false;
        static const char *const what[2][2] = {{"tau potential launch", ""}, {"tau potential launch (alpha)", "tau potential launch (beta)"}};
        ScopedTimer t(s, nspin == 2 ? "vxc_tau x2" : "vxc_tau");
        for (int sp = 0; sp < nspin; ++sp)
            if (!hip_ok(s, launch_vxc_tau(s->stream, vp, ngrid, nao, ao_grad, ct + (size_t)sp * 4 * ng, s->sync_slabs.d(), vxc[sp]), what[nspin - 1][sp]))
                return false;
    } else if (tau_term) {
        // the plain form, per spin: Q = c0 (plane in the AO slot) with c0 = ct_s and c1..c3 = 0, contracted with the same plane
        if (!reserve(s, s->sync_vtmp, sizeof(double) * nn, "hipMalloc(tau potential)", false)) return false;
        for (int sp = 0; sp < nspin; ++sp)
            if (!hip_ok(s, hipMemsetAsync(ct + (size_t)(4 * sp + 1) * ng, 0, sizeof(double) * 3 * ng, s->stream), "clear coefficients")) return false;
        for (int sp = 0; sp < nspin; ++sp)
            for (int k = 0; k < 3; ++k) {
                if (!vxc_stage(s, P, false, ngrid, nao, ao_grad + (size_t)k * ng * nao, ct + (size_t)sp * 4 * ng, s->slabs.d(), s->sync_vtmp.d(), nullptr))
                    return false;
                if (!hip_ok(s, launch_meta_add(s->stream, (long)nn, s->sync_vtmp.d(), vxc[sp]), "tau potential add")) return false;
            }
    }
    double out = std::numeric_limits<double>::quiet_NaN();
    if (!hip_ok(s, hipMemcpyAsync(&out, exc, sizeof(double), hipMemcpyDeviceToHost, s->stream), "copy Exc") ||
        !hip_ok(s, hipStreamSynchronize(s->stream), "synchronise"))
        return false;
    *exc_host = out;
    if (std::isnan(out)) { set_error(s, "Exc is NaN after the %s completed (non-finite inputs)", E.what); return false; }
    return true;
}

// What an entry that reads a response slot checks first: prepared, and for these sizes (ngrid 0: the entry has none of its own)
bool fxc_slot_ok(XCSolver *s, const FxcSlot &f, const char *who, const char *prepare, const char *note, long ngrid, int nao)
{
    if (f.ngrid <= 0) {
        set_error(s, "%s before %s%s", who, prepare, note);
        return false;
    }
    if (ngrid && (ngrid != f.ngrid || nao != f.nao)) {
        set_error(s, "%s sizes ngrid=%ld nao=%d differ from %s's ngrid=%ld nao=%d", who, ngrid, nao, prepare, f.ngrid, f.nao);
        return false;
    }
    return true;
}

// Linear response of Vxc, first half: the ground-state density step of a sweep (never the one-kernel plan for small
// bases: that one keeps no density) and the derivative table of the functional at that density.
// kind 0: the shipped formulas differentiated (DFT_FxcPrepare); 1, 2: the tables of the spin-resolved energy bodies
// (DFT_FxcPrepareSpin, which vouches for the kind), each in its own slot.
bool fxc_prepare(XCSolver *s, long ngrid, int nao, int nocc, const double *cocc, const double *dm, const double *ao,
                 const double *ao_grad, const double *w, int kind = 0)
{
    FxcSlot &f = s->fxc[kind];
    f.ngrid = 0;   // a failed Prepare leaves nothing to apply
    if (!enter(s, ngrid, nao, ao_grad)) return false;
    if (!ao || !w) { set_error(s, "DFT_FxcPrepare needs the AO values and the grid weights"); return false; }
    DensitySource src;
    if (!density_source(s, nao, dm, cocc, nocc, true, src)) return false;
    const bool gga = s->needs_grad;
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, false);
    const size_t ng = (size_t)ngrid;
    if (!reserve_dsym(s, P) || !reserve_planes(s, s->ws, true, ngrid, WS_SIGMA) ||
        !reserve(s, f.table, sizeof(double) * ng * (gga ? FXC_PLANES : 1), "hipMalloc(fxc table)") ||
        (gga && !reserve(s, f.g0[0], sizeof(double) * 3 * ng, "hipMalloc(fxc grad rho)")))
        return false;
    double *rho = s->ws.rho.d(), *sigma = s->ws.sigma.d();
    if (!run_density(s, P, src, ngrid, nao, ao, rho, f.g0[0].d(), sigma)) return false;   // grad rho goes straight to its keep
    if (kind == 0) {
        ScopedTimer t(s, "fxc_table");
        if (!hip_ok(s, launch_fxc_table(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, rho, gga ? sigma : nullptr, w, f.table.d(), s->quirks),
                    "response table launch"))
            return false;
    } else {
        ScopedTimer t(s, "fxc_table_spin");
        if (!hip_ok(s, launch_fxc_table_spin(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, rho, gga ? sigma : nullptr, w, f.table.d(), kind),
                    "spin response table launch"))
            return false;
    }
    if (!hip_ok(s, hipGetLastError(), "response prepare launch")) return false;
    f.ngrid = ngrid;
    f.nao = nao;
    return true;
}

// Second half: V1 of a perturbation dm1 -- its density through the same kernels (linear in the matrix), the response
// coefficients from the table, and the sweep's contraction and reduce.  Asynchronous on the solver's stream.
bool fxc_apply(XCSolver *s, long ngrid, int nao, const double *dm1, const double *ao, const double *ao_grad, double *v1, int kind = 0)
{
    static const char *const who[3] = {"DFT_FxcApply", "DFT_FxcApplyKind(kind=1)", "DFT_FxcApplyKind(kind=2)"};
    if (!enter(s, ngrid, nao, ao_grad)) return false;
    if (kind < 0 || kind > 2) { set_error(s, "DFT_FxcApplyKind: unknown kind %d (0 the DFT_FxcPrepare table, 1 triplet, 2 singlet through the spin-resolved bodies)", kind); return false; }
    const FxcSlot &f = s->fxc[kind];
    if (!fxc_slot_ok(s, f, who[kind], kind ? "DFT_FxcPrepareSpin" : "DFT_FxcPrepare",
                     kind ? " of that kind" : " (or the table was invalidated by an option change)", ngrid, nao))
        return false;
    if (!dm1 || !ao || !v1) { set_error(s, "DFT_FxcApply needs dm1, the AO values and the output matrix"); return false; }
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, false);
    const Planes &p = s->ws;
    if (!reserve_dsym(s, P) || !reserve_planes(s, s->ws, true, ngrid, WS_ALL) || !reserve_slabs(s, P, nao)) return false;
    launch_density(s, P, ngrid, nao, dm1, ao, s->dsym.d(), p.rho.d(), p.grad.d(), p.sigma.d());
    {
        ScopedTimer t(s, "fxc_coef");
        if (!hip_ok(s, launch_fxc_coef(s->stream, P.gga, ngrid, f.table.d(), f.g0[0].d(), p.rho.d(), p.grad.d(), p.coef.d()),
                    "response coefficient launch"))
            return false;
    }
    return vxc_stage(s, P, false, ngrid, nao, ao, p.coef.d(), s->slabs.d(), v1, nullptr);
}

// Open-shell response of Vxc, first half (DFT_FxcPrepareSpinPol): the density kernels on dm0_a, then on dm0_b, as
// DFT_ComputeXCSpin runs them, and the second-derivative table of the energy at that point (xc_response_pol.hip).  The
// table and the two gradients stay in a slot of their own; the densities pass through the synchronous entries' planes.
bool fxc_prepare_spinpol(XCSolver *s, long ngrid, int nao, const double *dm_a, const double *dm_b, const double *ao,
                         const double *ao_grad, const double *w)
{
    FxcSlot &f = s->fxc_pol;
    f.ngrid = 0;   // a failed Prepare leaves nothing to apply
    if (!enter(s, ngrid, nao, ao_grad)) return false;
    if (!dm_a || !dm_b || !ao || !w) {
        set_error(s, "DFT_FxcPrepareSpinPol needs both density matrices, the AO values and the grid weights");
        return false;
    }
    if (!spin_quirks_ok(s, "DFT_FxcPrepareSpinPol")) return false;
    const bool gga = s->needs_grad;
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, false);
    const size_t ng = (size_t)ngrid;
    if (!reserve_dsym(s, P) || !reserve_planes(s, s->sync_ws[0], false, ngrid, WS_SIGMA) || !reserve_planes(s, s->sync_ws[1], false, ngrid, 0) ||
        !reserve(s, f.table, sizeof(double) * ng * fxc_pol_planes(gga), "hipMalloc(fxc pol table)", false))
        return false;
    for (int k = 0; k < 2; ++k)
        if (gga && !reserve(s, f.g0[k], sizeof(double) * 3 * ng, "hipMalloc(fxc pol grad rho)", false)) return false;
    double *g_a = f.g0[0].d(), *g_b = f.g0[1].d();   // the gradients go straight to their keep
    launch_density_spin(s, P, ngrid, nao, dm_a, dm_b, ao, g_a, g_b);
    {
        ScopedTimer t(s, "fxc_table_pol");
        if (!hip_ok(s, launch_fxc_table_pol(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, s->sync_ws[0].rho.d(), s->sync_ws[1].rho.d(),
                                            gga ? g_a : nullptr, gga ? g_b : nullptr, w, f.table.d()), "open-shell response table launch"))
            return false;
    }
    f.ngrid = ngrid;
    f.nao = nao;
    return true;
}

// Second half (DFT_FxcApplySpinPol): the densities of dm1_a and dm1_b, the coupled coefficients of the two spins from
// the table, and the sweep's contraction and reduce once per spin.  Asynchronous on the solver's stream.
bool fxc_apply_spinpol(XCSolver *s, long ngrid, int nao, const double *dm1_a, const double *dm1_b, const double *ao,
                       const double *ao_grad, double *v1_a, double *v1_b)
{
    const FxcSlot &f = s->fxc_pol;
    if (!enter(s, ngrid, nao, ao_grad) || !fxc_slot_ok(s, f, "DFT_FxcApplySpinPol", "DFT_FxcPrepareSpinPol", "", ngrid, nao)) return false;
    if (!dm1_a || !dm1_b || !ao || !v1_a || !v1_b) {
        set_error(s, "DFT_FxcApplySpinPol needs both perturbations, the AO values and both output matrices");
        return false;
    }
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, ao_grad, false);
    Planes &a = s->sync_ws[0], &b = s->sync_ws[1];
    if (!reserve_dsym(s, P) || !reserve_slabs(s, P, nao) || !reserve_planes(s, a, false, ngrid, WS_ALL) ||
        !reserve_planes(s, b, false, ngrid, WS_COEF | WS_GRAD))
        return false;
    launch_density_spin(s, P, ngrid, nao, dm1_a, dm1_b, ao, a.grad.d(), b.grad.d());
    {
        ScopedTimer t(s, "fxc_coef_pol");
        if (!hip_ok(s, launch_fxc_coef_pol(s->stream, P.gga, ngrid, f.table.d(), f.g0[0].d(), f.g0[1].d(), a.rho.d(), b.rho.d(), a.grad.d(),
                                           b.grad.d(), a.coef.d(), b.coef.d()), "open-shell response coefficient launch"))
            return false;
    }
    if (!vxc_stage(s, P, false, ngrid, nao, ao, a.coef.d(), s->slabs.d(), v1_a, nullptr)) return false;
    return vxc_stage(s, P, false, ngrid, nao, ao, b.coef.d(), s->slabs.d(), v1_b, nullptr);
}

// J and/or K from rows (i, j), i in [i0, i0 + ni), of the dense ERI; `eri` points at row (i0, 0).
// i0 = 0, ni = nao is the reference's whole-matrix contraction; a proper sub-range is one rank's share of
// the row sharding: partial J over all columns, rows [i0, i0 + ni) of K, zeros elsewhere.
void jk(XCSolver *s, int nao, const double *eri, const double *dm, double *J, double *K, int i0 = 0, int ni = -1)
{
    s->last_error.clear();
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return; }
    if (nao <= 0 || nao > JK_COLS) { set_error(s, "dense-ERI J/K needs 1 <= nao <= %d (got %d)", JK_COLS, nao); return; }
    if (ni < 0) ni = nao;
    if (i0 < 0 || ni <= 0 || i0 + ni > nao) { set_error(s, "dense-ERI J/K: bad row range [%d, %d) of %d", i0, i0 + ni, nao); return; }
    if (!J && !K) return;
    const int n = nao;
    const size_t N2 = (size_t)n * n;
    const int KB = std::max(1, std::min(n, JK_COLS / n));
    const int ncb = (n + KB - 1) / KB;
    // (below ~48 functions the whole pass is a handful of workgroups either way and the symmetric kernels' extra slab sums
    //  cost more than their bytes save: H2O/def2-SVP 39 against 30 us)
    if (J && !K && s->eri_sym == 2 && i0 == 0 && ni == n && n >= 48) {   // the unique eighth only (k_j_sym8)
        const size_t NPK = (size_t)n * (n + 1) / 2;
        // packed columns per thread (4, 2, 1): the widest blocks that still leave more live workgroups than CUs (half of the
        // (block, chunk) pairs are live; measured: nao 114 -> 4 (52.9 us; 1: 67.2), nao 80 -> 1 (31.5 us; 4: 41.7))
        const int nchunk = (int)((NPK + JS8_RC - 1) / JS8_RC);
        int cpt = 4;
        while (cpt > 1 && (double)((NPK + 256 * cpt - 1) / (256 * cpt)) * nchunk / 2.0 < 1.2 * s->num_cu) cpt /= 2;
        {
            const char *ov = getenv("QCDFT_JSYM8_CPT");   // (tools/jsym_sweep.sh)
            if (ov && (atoi(ov) == 1 || atoi(ov) == 2 || atoi(ov) == 4)) cpt = atoi(ov);
        }
        const int ncb8 = (int)((NPK + 256 * cpt - 1) / (256 * cpt)), nslab = nchunk + ncb8;
        if (!reserve(s, s->jpart, sizeof(double) * (nslab + 1) * NPK, "hipMalloc(Jpart)")) return;
        double *jp = (double *)s->jpart.p;
        if (cpt == 4)      hipLaunchKernelGGL((k_j_sym8<4>), dim3(ncb8, nchunk), dim3(256), 0, s->stream, n, eri, dm, jp);
        else if (cpt == 2) hipLaunchKernelGGL((k_j_sym8<2>), dim3(ncb8, nchunk), dim3(256), 0, s->stream, n, eri, dm, jp);
        else               hipLaunchKernelGGL((k_j_sym8<1>), dim3(ncb8, nchunk), dim3(256), 0, s->stream, n, eri, dm, jp);
        hipLaunchKernelGGL(k_sum_slabs8_sym, dim3((unsigned)((NPK + 31) / 32)), dim3(256), 0, s->stream, n, nslab, jp, J);
        hip_ok(s, hipGetLastError(), "J launch");
        return;
    }
    if (J && !K && s->eri_sym && i0 == 0 && ni == n && n >= 48) {   // upper triangle only (k_j_sym)
        const int nslab = n + ncb;
        if (!reserve(s, s->jpart, sizeof(double) * nslab * N2, "hipMalloc(Jpart)")) return;
        double *jp = (double *)s->jpart.p;
        const bool vec = (n % 2 == 0) && (((uintptr_t)eri & 15) == 0);
        with_bool(vec, [&](auto V) { hipLaunchKernelGGL((k_j_sym<V>), dim3(ncb, n), dim3(256), 0, s->stream, n, KB, eri, dm, jp); });
        hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((N2 + 31) / 32)), dim3(256), 0, s->stream, N2, nslab, N2, jp, J);
        hip_ok(s, hipGetLastError(), "J launch");
        return;
    }
    // enough workgroups to fill the chip: split the j range when ni*ncb is small
    int jsplit = 1;
    while ((long)ni * ncb * jsplit < 4L * s->num_cu && jsplit * 2 <= n) jsplit *= 2;
    const int nslabJ = ni * jsplit;
    if (J && !reserve(s, s->jpart, sizeof(double) * nslabJ * N2, "hipMalloc(Jpart)")) return;
    if (K && !reserve(s, s->kpart, sizeof(double) * jsplit * (size_t)ni * n, "hipMalloc(Kpart)")) return;
    double *jp = (double *)s->jpart.p, *kp = (double *)s->kpart.p;
    dim3 g(ncb, ni * jsplit);
    hipStream_t st = s->stream;
    const bool vec = (n % 2 == 0) && (((uintptr_t)eri & 15) == 0);
    const auto launch = [&](auto WJ, auto WK) {
        with_bool(vec, [&](auto V) { hipLaunchKernelGGL((k_jk_stream<WJ, WK, V>), g, dim3(256), 0, st, n, KB, jsplit, i0, ni, eri, dm, jp, kp); });
    };
    if (J && K) launch(std::true_type{}, std::true_type{});
    else if (J) launch(std::true_type{}, std::false_type{});
    else        launch(std::false_type{}, std::true_type{});
    if (J) hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((N2 + 31) / 32)), dim3(256), 0, st, N2, nslabJ, N2, jp, J);
    if (K) {
        const size_t nk = (size_t)ni * n;
        if (ni != n) (void)hipMemsetAsync(K, 0, sizeof(double) * N2, st);
        hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((nk + 31) / 32)), dim3(256), 0, st, nk, jsplit, nk, kp, K + (size_t)i0 * n);
    }
    hip_ok(s, hipGetLastError(), "J/K launch");
}


// chunks per XCD for a split-K launch of `npair` output tiles: the count (<= 32) whose workgroup
// total fills whole rounds of the chip best, with slabs <= 2 GB and >= 64 contraction rows per chunk
long chunks_per_xcd(const XCSolver *s, int npair, long rows, size_t slab_bytes)
{
    // the fewest chunks whose workgroup total fills at least 92 % of whole rounds of the chip (more
    // chunks mean more slabs to sum and shorter contraction loops), else the best filling found
    long best_c = 1;
    double best = 0.0;
    for (long c = 1; c <= 32; ++c) {
        const long wgs = 8L * npair * c;
        if (8 * c * 64 > rows && c > 1) break;
        if ((double)(8 * c) * (double)slab_bytes > 2.0e9 && c > 1) break;
        const long rounds = (wgs + s->num_cu - 1) / s->num_cu;
        const double eff = (double)wgs / (double)(rounds * s->num_cu);
        if (eff >= 0.92) return c;
        if (eff > best + 1e-9) { best = eff; best_c = c; }
    }
    return best_c;
}

// Yt_P (nocc x nao, leading dimension ldy) = C^T L_P for every P: `c` (nao, nocc) is packed into cp (nao, ldp) first.
// dot: the tiles also leave the partials of v_P = Yt_P : C^T in vpart (k_gemm_tn's DOT).
void half_transform(hipStream_t st, int nao, int naux, int nocc, int ldp, int ldy, bool vecL, bool fused_dot,
                    const double *c, double *cp, const double *L, double *yt, double *vpart)
{
    const long n2 = (long)nao * nao;
    const int nBh = (nao + CD_BN - 1) / CD_BN;
    hipLaunchKernelGGL(k_pack_cocc, dim3((unsigned)(((long)nao * ldp + 255) / 256)), dim3(256), 0, st, nao, nocc, ldp, c, cp);
    // Yt_P (nocc x nao) = Cp^T L_P for every P
#define QCDFT_HALF3(WGM, MI, VL, DOT, NW)                                                                             \
    hipLaunchKernelGGL((k_gemm_tn<WGM, MI, true, VL, DOT, NW, (WGM == 1 ? 8 : 0), (WGM == 1 ? 4 : 0)>), g, dim3(64 * NW), 0, st, (long)nao, nocc, nao, ldp, nao, \
                       cp, 0L, L, n2, (long)nao, nBh, npair, 0, yt, ldy, (long)nocc * ldy, 0L, vpart)
#define QCDFT_HALF(WGM, MI, NW)                                                                                       \
    do {                                                                                                              \
        const int nA = (nocc + 64 * WGM - 1) / (64 * WGM), npair = nA * nBh;                                          \
        dim3 g((unsigned)((long)npair * naux));                                                                       \
        if (fused_dot) { if (vecL) QCDFT_HALF3(WGM, MI, true, true, NW); else QCDFT_HALF3(WGM, MI, false, true, NW); }   \
        else           { if (vecL) QCDFT_HALF3(WGM, MI, true, false, NW); else QCDFT_HALF3(WGM, MI, false, false, NW); } \
    } while (0)
    if (nocc <= 16) QCDFT_HALF(1, 1, 4);
    else if (nocc <= 32) QCDFT_HALF(1, 2, 4);
    else if (nocc <= 48) QCDFT_HALF(1, 3, 4);
    else if (nocc <= 64) QCDFT_HALF(1, 4, 4);
    else QCDFT_HALF(2, 4, 8);
#undef QCDFT_HALF
#undef QCDFT_HALF3
}

// J and/or K from Cholesky vectors L (naux, nao, nao), D = dm, dm = cocc cocc^T with cocc (nao, nocc)
int jk_factorized(XCSolver *s, int nao, int naux, int nocc, const double *L, const double *dm,
                  const double *cocc, double *J, double *K)
{
    s->last_error.clear();
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (nao <= 0 || naux <= 0 || !L) { set_error(s, "factorised J/K: bad sizes nao=%d naux=%d", nao, naux); return -1; }
    if (J && !dm) { set_error(s, "factorised J needs the density matrix"); return -1; }
    if (K && (!cocc || nocc <= 0)) { set_error(s, "factorised K needs occupied orbitals (nocc=%d)", nocc); return -1; }
    if (!J && !K) return 0;
    hipStream_t st = s->stream;
    const long n2 = (long)nao * nao;
    const int nB = (nao + CD_BN - 1) / CD_BN;
    // half transform: 64 x 256 tiles (8-row stages, four waves) while one 64-row tile holds all occupied orbitals,
    // 128 x 256 above; one partial of v_P per tile
    const int nBh = nB, npair_h = ((nocc + (nocc <= 64 ? 63 : 127)) / (nocc <= 64 ? 64 : 128)) * nBh;
    // v_P = L_P : D.  With K wanted too, the half transform leaves it as the dot of its result Yt_P with Cocc
    // (D = Cocc Cocc^T is the entry point's contract), one partial per tile; otherwise a pass of its own over L with D.
    const bool fused_dot = J && K;
    if (J) {
        if (!reserve(s, s->cdv, sizeof(double) * ((size_t)naux * (2 + npair_h) + 2), "hipMalloc(cd v)")) return -1;
        if (!fused_dot) {
            ScopedTimer t(s, "cd_dot");
            hipLaunchKernelGGL(k_cd_dot, dim3((unsigned)naux), dim3(256), 0, st, n2, L, dm, (double *)s->cdv.p);
        }
    }
    double *v = (double *)s->cdv.p, *vpart = v ? v + naux : nullptr;
    if (K) {
        const int ldp = ((nocc + 15) / 16) * 16;          // padded occupied dimension of the A operand
        const int ldy = (nao + 1) & ~1;                   // even leading dimension of Yt: 16-byte rows
        const long G = (long)naux * nocc;                 // rows of Yt
        const int nA2 = (nao + 127) / 128, npair2 = nA2 * nB;
        int live2 = 0; // tiles of K = Yt^T Yt that are computed (the rest are mirrored)
        for (int ia = 0; ia < nA2; ++ia)
            for (int ib = 0; ib < nB; ++ib) live2 += !(128 * ia >= CD_BN * ib + CD_BN);
        long per_xcd = s->ksplit > 0 ? s->ksplit : chunks_per_xcd(s, live2, G, sizeof(double) * (size_t)n2);
        while ((double)((G + 8 * per_xcd - 1) / (8 * per_xcd) + CD_BK) * ldy * 8.0 >= 4294967296.0) per_xcd *= 2; // a chunk of Yt stays below 4 GiB (one buffer descriptor)
        const int nslab = (int)(8 * per_xcd);
        long chunk = (G + nslab - 1) / nslab;
        chunk = ((chunk + CD_BK - 1) / CD_BK) * CD_BK;
        const bool fresh = sizeof(double) * (size_t)G * ldy > s->cdy.cap;
        if (!reserve(s, s->cdc, sizeof(double) * (size_t)nao * ldp, "hipMalloc(cd cocc)") ||
            !reserve(s, s->cdy, sizeof(double) * (size_t)G * ldy, "hipMalloc(cd Yt)") ||
            !reserve(s, s->kpart, sizeof(double) * (size_t)nslab * n2, "hipMalloc(cd K slabs)"))
            return -1;
        double *cp = (double *)s->cdc.p, *yt = (double *)s->cdy.p, *kp = (double *)s->kpart.p;
        if (fresh && ldy != nao) // the pad column is read (into discarded outputs) but never written
            if (!hip_ok(s, hipMemsetAsync(yt, 0, s->cdy.cap, st), "memset(cd Yt)")) return -1;
        const bool vecL = (nao % 2 == 0) && (((uintptr_t)L & 15) == 0);
        {
            ScopedTimer t(s, "cd_half");
            half_transform(st, nao, naux, nocc, ldp, ldy, vecL, fused_dot, cocc, cp, L, yt, vpart);
        }
        {
            ScopedTimer t(s, "cd_k");
            // K = Yt^T Yt, split over the (P, i) rows
            dim3 g((unsigned)(nslab * live2));
            hipLaunchKernelGGL((k_gemm_tn<2, 4, true, true>), g, dim3(BG_THREADS), 0, st, G, nao, nao, ldy, ldy,
                               yt, 0L, yt, 0L, chunk, nB, live2, 1, kp, nao, 0L, n2, (double *)nullptr, 1);
            hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((n2 + 31) / 32)), dim3(256), 0, st, (size_t)n2, nslab, (size_t)n2, kp, K);
            if (live2 < npair2)
                hipLaunchKernelGGL(k_mirror_lower, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, nao, K);
        }
    }
    if (J) {
        ScopedTimer t(s, "cd_j");
        // J = sum_P v_P L_P: slices of vectors so that the pass has >= ~4 workgroups per CU
        const long eb = (n2 + 255) / 256;
        int nsl = (int)std::max<long>(1, std::min<long>(naux, (4L * s->num_cu + eb - 1) / eb));
        const int pslice = (naux + nsl - 1) / nsl;
        nsl = (naux + pslice - 1) / pslice;
        if (!reserve(s, s->jpart, sizeof(double) * (size_t)nsl * n2, "hipMalloc(cd J slabs)")) return -1;
        double *jp = (double *)s->jpart.p;
        if (fused_dot) {
            // The fused dots are L_P : (cocc cocc^T).  A dm that is NOT that product (damped, mixed, fractional occupations)
            // must give ITS Coulomb matrix: checked on the device, and v_P = L_P : dm is then taken in a pass of its own
            // (a launch that exits at once when the two agree) -- no host round trip either way.
            double *vdot = vpart + (size_t)naux * npair_h;
            int *flag = (int *)(vdot + naux);
            (void)hipMemsetAsync(flag, 0, sizeof(int), st);
            hipLaunchKernelGGL(k_dm_consistency, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, nao, nocc, dm, cocc, flag);
            hipLaunchKernelGGL(k_cd_dot_if, dim3((unsigned)naux), dim3(256), 0, st, flag, n2, L, dm, vdot);
            hipLaunchKernelGGL(k_cd_vsum, dim3((unsigned)((naux + 255) / 256)), dim3(256), 0, st, naux, npair_h, vpart, v, flag, vdot);
        }
        hipLaunchKernelGGL(k_cd_axpy, dim3((unsigned)eb, (unsigned)nsl), dim3(256), 0, st, n2, naux, pslice, L, v, jp, nao);
        hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((n2 + 31) / 32)), dim3(256), 0, st, (size_t)n2, nsl, (size_t)n2, jp, J);
        hipLaunchKernelGGL(k_sym_from_upper, dim3((unsigned)eb), dim3(256), 0, st, nao, J);
    }
    return hip_ok(s, hipGetLastError(), "factorised J/K launch") ? 0 : -1;
}

// Response J and M of nvec trial densities that share their left factor (DFT_ComputeJKFactorizedResponse):
//     J_k = J[A B_k^T + B_k A^T],   M_k = sum_P (L_P A)(L_P B_k)^T   (K[A B_k^T +- B_k A^T] = M_k +- M_k^T)
// A (nao, nocc), B (nvec, nao, nocc).  Cost: ONE half transform of A per call; v[k][P] = L_P : D_k from Yt^A, not from
// L; one pass over L per group of up to CDR_MAXV trials for J; per trial of M one half transform of B_k and one
// Yt^A^T Yt^B_k product with every tile live.  No slicing below depends on nvec or on k: a trial's J and M are
// bitwise the same alone or in any batch.
int jk_factorized_response(XCSolver *s, int nao, int naux, int nocc, int nvec, const double *L, const double *A,
                           const double *B, double *J, double *M)
{
    s->last_error.clear();
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (nao <= 0 || naux <= 0 || nocc <= 0 || nvec <= 0) {
        set_error(s, "factorised response J/K: bad sizes nao=%d naux=%d nocc=%d nvec=%d", nao, naux, nocc, nvec);
        return -1;
    }
    if (!L || !A || !B) { set_error(s, "factorised response J/K needs the vectors and both factors"); return -1; }
    if (!J && !M) return 0;
    hipStream_t st = s->stream;
    const long n2 = (long)nao * nao;
    const size_t nb = (size_t)nao * nocc;                 // doubles of one factor
    const int nB = (nao + CD_BN - 1) / CD_BN;
    const int ldp = ((nocc + 15) / 16) * 16, ldy = (nao + 1) & ~1;
    const long G = (long)naux * nocc;
    const bool vecL = (nao % 2 == 0) && (((uintptr_t)L & 15) == 0);
    const size_t ybytes = sizeof(double) * (size_t)G * ldy;
    const bool fresh = ybytes > s->cdy.cap;
    if (!reserve(s, s->cdc, sizeof(double) * (size_t)nao * ldp, "hipMalloc(cd cocc)") ||
        !reserve(s, s->cdy, ybytes, "hipMalloc(cd Yt)"))
        return -1;
    double *cpa = (double *)s->cdc.p, *yta = (double *)s->cdy.p;
    if (fresh && ldy != nao) // the pad column is read (into discarded outputs) but never written
        if (!hip_ok(s, hipMemsetAsync(yta, 0, s->cdy.cap, st), "memset(cd Yt)")) return -1;
    {
        ScopedTimer t(s, "cdr_half");
        half_transform(st, nao, naux, nocc, ldp, ldy, vecL, false, A, cpa, L, yta, nullptr);
    }
    if (J) {
        const int gmax = std::min(nvec, CDR_MAXV);
        const int ept = vecL ? 2 : 1;
        const long eb = (n2 + 256 * ept - 1) / (256 * ept);
        // slices of vectors so that the pass has >= ~4 workgroups per CU (from nao, naux and the device alone)
        int nsl = (int)std::max<long>(1, std::min<long>(naux, (4L * s->num_cu + eb - 1) / eb));
        const int pslice = (naux + nsl - 1) / nsl;
        nsl = (naux + pslice - 1) / pslice;
        if (!reserve(s, s->cdv, sizeof(double) * (size_t)naux * gmax, "hipMalloc(cd v)") ||
            !reserve(s, s->cdbt, sizeof(double) * nb * gmax, "hipMalloc(cd B^T)") ||
            !reserve(s, s->jpart, sizeof(double) * (size_t)gmax * nsl * n2, "hipMalloc(cd J slabs)"))
            return -1;
        double *v = (double *)s->cdv.p, *bt = (double *)s->cdbt.p, *jp = (double *)s->jpart.p;
        const dim3 gdot((unsigned)naux), gax((unsigned)eb, (unsigned)nsl), gtr((unsigned)((nb + 255) / 256), 1);
        for (int k0 = 0; k0 < nvec; k0 += CDR_MAXV) {
            const int nv = std::min(CDR_MAXV, nvec - k0);
            {
                ScopedTimer t(s, "cdr_dot");
                hipLaunchKernelGGL(k_cdr_transpose, dim3(gtr.x, (unsigned)nv), dim3(256), 0, st, nao, nocc, B + (size_t)k0 * nb, bt);
#define QCDFT_CDR_DOT(NV) case NV: hipLaunchKernelGGL((k_cdr_dot<NV>), gdot, dim3(256), 0, st, nao, nocc, ldy, naux, yta, bt, v); break
                switch (nv) {
                    QCDFT_CDR_DOT(1); QCDFT_CDR_DOT(2); QCDFT_CDR_DOT(3); QCDFT_CDR_DOT(4);
                    QCDFT_CDR_DOT(5); QCDFT_CDR_DOT(6); QCDFT_CDR_DOT(7); QCDFT_CDR_DOT(8);
                }
#undef QCDFT_CDR_DOT
            }
            ScopedTimer t(s, "cdr_j");
#define QCDFT_CDR_AXPY(NV)                                                                                                      \
    case NV:                                                                                                                    \
        if (vecL) hipLaunchKernelGGL((k_cdr_axpy<NV, true>), gax, dim3(256), 0, st, n2, nao, naux, pslice, nsl, L, v, jp);       \
        else      hipLaunchKernelGGL((k_cdr_axpy<NV, false>), gax, dim3(256), 0, st, n2, nao, naux, pslice, nsl, L, v, jp);      \
        break
            switch (nv) {
                QCDFT_CDR_AXPY(1); QCDFT_CDR_AXPY(2); QCDFT_CDR_AXPY(3); QCDFT_CDR_AXPY(4);
                QCDFT_CDR_AXPY(5); QCDFT_CDR_AXPY(6); QCDFT_CDR_AXPY(7); QCDFT_CDR_AXPY(8);
            }
#undef QCDFT_CDR_AXPY
            for (int k = 0; k < nv; ++k) {
                double *Jk = J + (size_t)(k0 + k) * n2;
                hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((n2 + 31) / 32)), dim3(256), 0, st, (size_t)n2, nsl, (size_t)n2,
                                   jp + (size_t)k * nsl * n2, Jk);
                hipLaunchKernelGGL(k_sym_from_upper, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, nao, Jk);
            }
        }
    }
    if (M) {
        const int npair2 = ((nao + 127) / 128) * nB;      // every tile of Yt^A^T Yt^B is live: the product is not symmetric
        long per_xcd = s->ksplit > 0 ? s->ksplit : chunks_per_xcd(s, npair2, G, sizeof(double) * (size_t)n2);
        while ((double)((G + 8 * per_xcd - 1) / (8 * per_xcd) + CD_BK) * ldy * 8.0 >= 4294967296.0) per_xcd *= 2; // a chunk of Yt stays below 4 GiB
        const int nslab = (int)(8 * per_xcd);
        long chunk = (G + nslab - 1) / nslab;
        chunk = ((chunk + CD_BK - 1) / CD_BK) * CD_BK;
        const bool fresh2 = ybytes > s->cdy2.cap;
        if (!reserve(s, s->cdc2, sizeof(double) * (size_t)nao * ldp, "hipMalloc(cd right factor)") ||
            !reserve(s, s->cdy2, ybytes, "hipMalloc(cd Yt of the right factor)") ||
            !reserve(s, s->kpart, sizeof(double) * (size_t)nslab * n2, "hipMalloc(cd K slabs)"))
            return -1;
        double *cpb = (double *)s->cdc2.p, *ytb = (double *)s->cdy2.p, *kp = (double *)s->kpart.p;
        if (fresh2 && ldy != nao)
            if (!hip_ok(s, hipMemsetAsync(ytb, 0, s->cdy2.cap, st), "memset(cd Yt of the right factor)")) return -1;
        ScopedTimer t(s, "cdr_m");
        for (int k = 0; k < nvec; ++k) {
            half_transform(st, nao, naux, nocc, ldp, ldy, vecL, false, B + (size_t)k * nb, cpb, L, ytb, nullptr);
            hipLaunchKernelGGL((k_gemm_tn<2, 4, true, true>), dim3((unsigned)(nslab * npair2)), dim3(BG_THREADS), 0, st, G, nao, nao, ldy, ldy,
                               yta, 0L, ytb, 0L, chunk, nB, npair2, 1, kp, nao, 0L, n2, (double *)nullptr, 0);
            hipLaunchKernelGGL(k_sum_slabs8, dim3((unsigned)((n2 + 31) / 32)), dim3(256), 0, st, (size_t)n2, nslab, (size_t)n2, kp,
                               M + (size_t)k * n2);
        }
    }
    return hip_ok(s, hipGetLastError(), "factorised response J/K launch") ? 0 : -1;
}

// dm = L L^T on the device (dm_factor.hip): the rank (>= 1) with L (nao, rank) C-order in `out` (nao * max_rank doubles),
// 0 when dm is not such a product with rank <= max_rank (info[2] says why), -1 on an error.  Synchronous: the rank decides
// what is launched next, and the acceptance flag is the answer.  Accepted means k_dm_consistency -- the bound the
// factorised J/K build already trusts -- found |dm - L L^T| within round-off over the WHOLE matrix: the factorisation
// itself reads pivot rows only, so this is also what rejects a non-symmetric dm.
int factor_density(XCSolver *s, int nao, const double *dm, int max_rank, double tol, double *out, double *info)
{
    double st4[DMF_STATUS_DOUBLES] = {0.0, 0.0, (double)DMF_SIZE, 0.0};
    auto done = [&](int rc) {
        if (info) std::copy(st4, st4 + DMF_STATUS_DOUBLES, info);
        return rc;
    };
    s->last_error.clear();
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return done(-1); }
    if (nao <= 0 || !dm || !out) { set_error(s, "density factorisation: bad arguments (nao=%d)", nao); return done(-1); }
    if (nao < DMF_MIN_NAO || nao > DMF_MAX_NAO) return done(0);
    if (max_rank <= 0) max_rank = nao / 2;
    max_rank = std::min(max_rank, nao);
    if (!(tol > 0.0)) tol = 1e-13;
    if (!reserve(s, s->dmf_lt, sizeof(double) * (size_t)max_rank * nao, "hipMalloc(dm factor)") ||
        !reserve(s, s->dmf_st, sizeof(double) * (DMF_STATUS_DOUBLES + 1), "hipMalloc(dm factor status)"))
        return done(-1);
    hipStream_t st = s->stream;
    double *Lt = (double *)s->dmf_lt.p, *dst = (double *)s->dmf_st.p;
    int *flag = (int *)(dst + DMF_STATUS_DOUBLES);
    {
        ScopedTimer t(s, "dm_factor");
        if (!hip_ok(s, launch_dm_factor(st, nao, max_rank, tol, dm, Lt, dst), "density factorisation launch")) return done(-1);
    }
    if (!hip_ok(s, hipMemcpyAsync(st4, dst, sizeof st4, hipMemcpyDeviceToHost, st), "copy factorisation status") ||
        !hip_ok(s, hipStreamSynchronize(st), "density factorisation"))
        return done(-1);
    const int rank = (int)st4[0];
    if ((int)st4[2] != DMF_OK || rank < 1 || rank > max_rank) return done(0);
    int h_flag = 1;
    {
        ScopedTimer t(s, "dm_factor_check");
        (void)hipMemsetAsync(flag, 0, sizeof(int), st);
        if (!hip_ok(s, launch_dm_factor_pack(st, nao, rank, Lt, out), "factor pack launch")) return done(-1);
        const long n2 = (long)nao * nao;
        hipLaunchKernelGGL(k_dm_consistency, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, nao, rank, dm, (const double *)out, flag);
        if (!hip_ok(s, launch_dm_nonfinite(st, nao, dm, flag), "factor check launch")) return done(-1);
    }
    if (!hip_ok(s, hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st), "copy factorisation flag") ||
        !hip_ok(s, hipStreamSynchronize(st), "density factorisation check"))
        return done(-1);
    if (h_flag) {
        st4[2] = (double)DMF_INCONSISTENT;
        return done(0);
    }
    return done(rank);
}

// The AO shell table on the device: validated, packed and uploaded once per distinct table
// ([AoShell x nshell][exp x nprim][coef x nprim][AoChunk x nchunk][order x nshell]).
struct AoTable {
    const AoShell *sh; const double *exp, *coef; const AoChunk *chunks; const int *order;
    int nshell, nprim, nchunk, maxcol; bool even_blocks;
};

bool prepare_ao_table(XCSolver *s, int nao, int nshell, const double *shl_xyz, const int *shl_l, const int *shl_nprim,
                      const int *shl_off, const int *shl_ao, const double *prim_exp, const double *prim_coef, int nprim_total,
                      AoTable &out)
{
    if (nao <= 0 || nshell <= 0 || nprim_total <= 0) {
        set_error(s, "bad AO sizes");
        return false;
    }
    int next_col = 0;
    std::vector<AoChunk> chunks;
    for (int i = 0; i < nshell; ++i) {
        const int l = shl_l[i], nf = 2 * l + 1;
        if (l < 0 || l > AO_MAX_L) { set_error(s, "shell %d: l=%d unsupported (max %d)", i, l, AO_MAX_L); return false; }
        if (shl_nprim[i] <= 0 || shl_off[i] < 0 || shl_off[i] + shl_nprim[i] > nprim_total) { set_error(s, "shell %d: primitive range out of bounds", i); return false; }
        if (shl_ao[i] != next_col) { set_error(s, "shell %d: AO columns must be contiguous and ascending (expected %d, got %d)", i, next_col, shl_ao[i]); return false; }
        if (chunks.empty()) {
            chunks.push_back(AoChunk{i, i, next_col, 0});
        } else if (chunks.back().ncol + nf > AO_CW) {
            // new column block; keep its first column even (16-byte stores) by taking the previous
            // shell along when needed -- every shell has an odd width, so that flips the parity
            AoChunk &b = chunks.back();
            if ((next_col & 1) && b.shell_hi - b.shell_lo >= 2) {
                const int pf = 2 * shl_l[i - 1] + 1;
                b.shell_hi -= 1;
                b.ncol -= pf;
                chunks.push_back(AoChunk{i - 1, i, next_col - pf, pf});
            } else {
                chunks.push_back(AoChunk{i, i, next_col, 0});
            }
        }
        chunks.back().shell_hi = i + 1;
        chunks.back().ncol += nf;
        next_col += nf;
    }
    if (next_col != nao) { set_error(s, "shell table covers %d AO columns, nao=%d", next_col, nao); return false; }
    const int nchunk = (int)chunks.size();
    int maxcol = 0;
    bool even = true;
    std::vector<int> order(nshell);
    for (const AoChunk &c : chunks) {
        maxcol = std::max(maxcol, c.ncol);
        if (c.col_lo & 1) even = false;
        for (int i = c.shell_lo; i < c.shell_hi; ++i) order[i] = i;
        std::stable_sort(order.begin() + c.shell_lo, order.begin() + c.shell_hi, [&](int a, int b) {
            return shl_l[a] != shl_l[b] ? shl_l[a] < shl_l[b] : shl_nprim[a] < shl_nprim[b];
        });
    }
    const size_t off_exp = sizeof(AoShell) * nshell;
    const size_t off_chunk = off_exp + 2 * sizeof(double) * nprim_total;
    const size_t off_order = off_chunk + sizeof(AoChunk) * nchunk;
    const size_t bytes = off_order + sizeof(int) * nshell;
    std::vector<unsigned char> blob(bytes);
    AoShell *sh = (AoShell *)blob.data();
    for (int i = 0; i < nshell; ++i) {
        sh[i].x = shl_xyz[3 * i]; sh[i].y = shl_xyz[3 * i + 1]; sh[i].z = shl_xyz[3 * i + 2];
        sh[i].l = shl_l[i]; sh[i].nprim = shl_nprim[i]; sh[i].off = shl_off[i]; sh[i].ao = shl_ao[i];
    }
    double *pe = (double *)(blob.data() + off_exp);
    memcpy(pe, prim_exp, sizeof(double) * nprim_total);
    memcpy(pe + nprim_total, prim_coef, sizeof(double) * nprim_total);
    memcpy(blob.data() + off_chunk, chunks.data(), sizeof(AoChunk) * nchunk);
    memcpy(blob.data() + off_order, order.data(), sizeof(int) * nshell);
    if (blob != s->shell_blob) {
        if (!reserve(s, s->shells, bytes, "hipMalloc(shells)")) return false;
        if (!hip_ok(s, hipMemcpyAsync(s->shells.p, blob.data(), bytes, hipMemcpyHostToDevice, s->stream), "upload shells") ||
            !hip_ok(s, hipStreamSynchronize(s->stream), "synchronise"))
            return false;
        s->shell_blob.swap(blob);
    }
    const unsigned char *base = (const unsigned char *)s->shells.p;
    out.sh = (const AoShell *)base;
    out.exp = (const double *)(base + off_exp);
    out.coef = out.exp + nprim_total;
    out.chunks = (const AoChunk *)(base + off_chunk);
    out.order = (const int *)(base + off_order);
    out.nshell = nshell; out.nprim = nprim_total; out.nchunk = nchunk; out.maxcol = maxcol; out.even_blocks = even;
    return true;
}

void launch_ao(XCSolver *s, const AoTable &t, long ngrid, int nao, const double *coords, double *ao, double *ao_grad)
{
    const bool vec = t.even_blocks && (nao % 2 == 0) && ((uintptr_t)ao % 16 == 0) && ((uintptr_t)ao_grad % 16 == 0);
    // 16 points per workgroup unless their LDS tile would leave fewer than three workgroups per CU
    // (measured, Benzene: def2-SVP deriv 1 139 -> 122 us with 8; STO-3G and deriv 0 are 10 % faster with 16)
    const int ao_pt = s->ao_pt ? s->ao_pt : ((ao_grad ? 4 : 1) * 16 * (t.maxcol | 1) * 8 > 53 * 1024 ? 8 : 16);
    launch_eval_ao(s->stream, ngrid, nao, t.nchunk, t.maxcol, vec, ao_pt, s->num_cu, t.nshell, t.nprim, t.sh, t.exp, t.coef, t.chunks, t.order,
                   coords, ao, ao_grad);
}

// V (+)= V_chunk, Exc (+)= Exc_chunk: the grid chunks of the direct sweep add up by linearity in the grid points
__global__ void k_accumulate_chunk(long n2, int add, const double *__restrict__ vc, const double *__restrict__ ec,
                                   double *__restrict__ v, double *__restrict__ e)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n2) v[i] = add ? v[i] + vc[i] : vc[i];
    if (i == 0) *e = add ? *e + *ec : *ec;
}

// What tells the eight gradient-side entries apart: the entry's name, its sentence for a null pointer, what a failed allocation
// of the padded matrices and of the slabs and a failed density or pointwise launch are called, the timer label of that
// pointwise kernel (the closed-shell gradient's is launch_xc_points' own), the number of spins and whether the entry forms
// tau.  A meta entry counts ao_grad and ao_hess among the pointers of `needs`; the others name them in sentences of their own.
struct XcgEntry {
    const char *who, *needs, *alloc_dp, *alloc_slabs, *density_launch, *launch, *timer;
    int nspin;
    bool meta;
};

// What the eight refuse first, in this order for every entry: the solver's kind, a null pointer, the sizes and a null ao_grad
// on a gradient-corrected solver (sizes_ok), for a gradient a
// null ao_hess on such a solver and a null ao_grad on any other, then quirks = 1 where the potentials are derivatives of the
// energy.  The callers go on with the LDS request (a gradient) and, last, the device: every fault of the arguments can be
// told apart from "no usable HIP device", and nothing has touched the device by then.
bool xcg_enter(XCSolver *s, const XcgEntry &E, bool gradient, long ngrid, int nao, const double *const dm[2], const double *ao,
               const double *w, const double *ao_grad, const double *ao_hess, const double *out)
{
    if (!enter_kind(s, 0, E.meta ? E.who : nullptr)) return false;
    bool ptrs = ao && out && (w || !gradient) && (!E.meta || (ao_grad && (ao_hess || !gradient)));
    for (int sp = 0; sp < E.nspin; ++sp) ptrs = ptrs && dm[sp];
    if (!ptrs) {
        set_error(s, "%s", E.needs);
        return false;
    }
    if (!sizes_ok(s, ngrid, nao, ao_grad)) return false;
    if (gradient && s->needs_grad && !ao_hess) { set_error(s, "ao_hess pointer is null for a gradient-corrected functional"); return false; }
    if (gradient && !ao_grad) { set_error(s, "%s needs ao_grad: the derivative of the density by a centre is made of it", E.who); return false; }
    return (E.nspin == 1 && !E.meta) || spin_quirks_ok(s, E.who);
}

// The set's buffers at the size of this call: `parts` of each spin's planes (sigma and `nxb` Exc partials with [0] alone), the
// padded matrix of each spin, and for a meta entry tau and, beside coefficient planes, ct.
bool reserve_xcg(XCSolver *s, const XcgEntry &E, const SweepPlan &P, long ngrid, unsigned parts, long nxb)
{
    const size_t ng = sizeof(double) * (size_t)ngrid * E.nspin;
    return reserve_planes(s, s->xcg[0], false, ngrid, parts, nxb) &&
           (E.nspin == 1 || reserve_planes(s, s->xcg[1], false, ngrid, parts & ~WS_SIGMA)) &&
           reserve(s, s->xcg_dp, sizeof(double) * E.nspin * P.NP * P.NP, E.alloc_dp, false) &&
           (!E.meta || (reserve(s, s->xcg_tau, ng, "hipMalloc(meta gradient tau)", false) &&
                        (!(parts & WS_COEF) || reserve(s, s->xcg_ct, ng, "hipMalloc(meta gradient tau coefficient)", false))));
}

// The density stage the eight share: the sweep's density kernels with the sweep's choices on each spin's matrix into that
// spin's planes; the padded symmetric matrix of each spin where something reads it back (`keep_dp`: k_xc_grad and k_tau do.
// The wave-specialised density kernel symmetrises dm itself, so k_sym_dm runs here on that plan; the other plans leave the
// matrix behind); and for a meta entry k_tau (two spins: k_tau_spin or, with "tau_spin_fused" = 0, k_tau once per spin) on
// that matrix -- compute_tau's launch half, without its second
// symmetrisation -- or, with both meta weights zero, the plane of zeros the pointwise kernels read.
bool xcg_density(XCSolver *s, const XcgEntry &E, const SweepPlan &P, bool keep_dp, long ngrid, int nao, const double *const dm[2],
                 const double *ao, const double *ao_grad)
{
    const size_t np2 = (size_t)P.NP * P.NP, ng = (size_t)ngrid;
    double *Dp = s->xcg_dp.d();
    for (int sp = 0; sp < E.nspin; ++sp)
        launch_density(s, P, ngrid, nao, dm[sp], ao, Dp + sp * np2, s->xcg[sp].rho.d(), s->xcg[sp].grad.d(), s->xcg[0].sigma.d());
    if (P.fast && keep_dp) {
        ScopedTimer t(s, "sym_dm");
        for (int sp = 0; sp < E.nspin; ++sp)
            hipLaunchKernelGGL(k_sym_dm, dim3(P.NP / 16, P.NP / 16), dim3(16, 16), 0, s->stream, nao, P.NP, dm[sp], Dp + sp * np2);
    }
    if (!hip_ok(s, hipGetLastError(), E.density_launch)) return false;
    if (!E.meta) return true;
    double *const tau[2] = {s->xcg_tau.d(), s->xcg_tau.d() + ng};
    if (!s->meta_active) return hip_ok(s, hipMemsetAsync(tau[0], 0, sizeof(double) * E.nspin * ng, s->stream), "clear tau");
    const bool both = E.nspin == 2 && s->tau_spin_fused;   // as compute_tau chooses: k_tau_spin, or k_tau once per spin
    const TauPlan tp = both ? tau_spin_plan(s->num_cu, ngrid, nao) : tau_plan(s->num_cu, ngrid, nao);   // tp.NP = P.NP
    ScopedTimer t(s, E.nspin == 1 ? "tau" : both ? "tau_spin" : "tau x2");
    return launch_tau_stage(s, tp, both, E.nspin, ngrid, nao, ao_grad, Dp, tau);
}

// XC part of the nuclear gradient: DFT_ComputeXCGradient, DFT_ComputeXCGradientSpin, DFT_ComputeXCGradientMeta and
// DFT_ComputeXCGradientMetaSpin, each stage once over sp < nspin.  The density stage above, the pointwise kernel of the
// entry's sweep exactly as that sweep runs it (launch_xc_points, xc_spin.hip, xc_meta.hip, xc_meta_spin.hip), then the
// contraction of every spin's (coefficient planes, padded matrix)
// pair with the ten planes and a fixed-order slab sum: k_xc_grad; for two spins both pairs in one launch or, with option
// "xcg_spin_fused" = 0, one launch per spin into two slab sets; for a meta-GGA k_xc_grad_meta<true> with c0..c3 and ct in one
// pass or, with "xcg_meta_fused" = 0, k_xc_grad and k_xc_grad_meta<false> into two slab sets; for a meta-GGA at two spins
// k_xc_grad_meta_spin with both spins' c0..c3 and ct in one pass or, with "xcg_meta_spin_fused" = 0, that plain pair once per
// spin into four slab sets.  With both meta weights zero the tau stage and the tau term are left out: k_xc_grad alone, as
// DFT_ComputeXCGradient or DFT_ComputeXCGradientSpin runs it.  Never the one-kernel plan
// for small bases (it keeps no coefficients), never recorded; asynchronous on the solver's stream.
bool xc_gradient(XCSolver *s, const XcgEntry &E, long ngrid, int nao, const double *const dm[2], const double *ao, const double *w,
                 const double *ao_grad, const double *ao_hess, double *out)
{
    if (!xcg_enter(s, E, true, ngrid, nao, dm, ao, w, ao_grad, ao_hess, out)) return false;
    const bool spin = E.nspin == 2, gga = s->needs_grad, tau_term = E.meta && s->meta_active;
    const bool fused = !tau_term ? spin && s->xcg_spin_fused != 0 : spin ? s->xcg_meta_spin_fused != 0 : s->xcg_meta_fused != 0;
    const XcGradPlan G = xc_grad_plan(s->num_cu, gga, spin && fused && !tau_term ? 2 : 1, ngrid, nao);        // k_xc_grad
    const XcGradPlan T = !tau_term ? XcGradPlan{}
                         : spin && fused ? xc_grad_meta_spin_plan(s->num_cu, ngrid, nao)                        // k_xc_grad_meta_spin
                                         : xc_grad_meta_plan(s->num_cu, fused, ngrid, nao);                     // k_xc_grad_meta<fused>
    const size_t lds = !tau_term ? G.lds : fused ? T.lds : std::max(G.lds, T.lds);
    if (lds > 160 * 1024) {
        set_error(s, "%s: nao=%d needs %zu bytes of LDS per workgroup%s", E.who, nao, lds, E.meta ? ", above the 160 KB a workgroup has" : "");
        return false;
    }
    if (!device_ready(s)) return false;
    // an LDA-class solver's density kernels read ao_grad's first plane pointer only as a dummy: plan as the sweep does
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, gga ? ao_grad : nullptr, false);
    const long nxb = E.meta ? meta_points_blocks(ngrid) : spin ? spin_points_blocks(ngrid) : (ngrid + 255) / 256;
    const int nslab = !tau_term ? (spin && !fused ? 2 : 1) * G.nwg : fused ? T.nwg : E.nspin * (G.nwg + T.nwg);
    if (!reserve_xcg(s, E, P, ngrid, WS_ALL, nxb) ||
        !reserve(s, s->xcg_slabs, sizeof(double) * (size_t)nslab * 3 * nao, E.alloc_slabs, false) ||
        !xcg_density(s, E, P, true, ngrid, nao, dm, ao, ao_grad))
        return false;
    const Planes &a = s->xcg[0], &b = s->xcg[1];   // sigma and the Exc partials with [0] alone
    const double *Da = s->xcg_dp.d(), *Db = Da + (size_t)P.NP * P.NP;
    double *ct = s->xcg_ct.d(), *ctb = ct + (size_t)ngrid, *slabs = s->xcg_slabs.d();   // ctb: two spins with tau alone
    const double *taua = s->xcg_tau.d(), *taub = taua + (size_t)ngrid;
    if (!spin && !E.meta) {   // the pointwise kernel: the first of the two stages that differ in more than their loop count
        launch_xc_points(s, ngrid, nxb, w, a);
        if (!hip_ok(s, hipGetLastError(), E.launch)) return false;
    } else {
        ScopedTimer t(s, E.timer);
        const hipError_t e =
            E.meta && spin ? launch_xc_points_meta_spin(s->stream, s->mix.c, s->meta, ngrid, a.rho.d(), b.rho.d(), a.grad.d(), b.grad.d(), taua, taub, w,
                                                        a.coef.d(), b.coef.d(), ct, ctb, a.partial.d())
            : E.meta ? launch_xc_points_meta(s->stream, s->mix.c, s->meta, ngrid, a.rho.d(), a.grad.d(), taua, w, a.coef.d(), ct, a.partial.d())
                   : launch_xc_points_spin(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, a.rho.d(), b.rho.d(), gga ? a.grad.d() : nullptr,
                                           gga ? b.grad.d() : nullptr, w, a.coef.d(), b.coef.d(), a.partial.d());
        if (!hip_ok(s, e, E.launch)) return false;
    }
    // ... and the contraction.  One-sided types hand over c0 = w vrho, c_k = 4 w vsigma grad_k rho; B3LYP half of each (its M + M^T)
    const double fac = s->type == SOLVER_B3LYP ? 2.0 : 1.0;
    struct Form { const char *timer, *what; };
    const Form form = tau_term && spin ? (fused ? Form{"xc_grad_meta_spin", "spin meta XC gradient launch (fused)"}
                                                : Form{"xc_grad + xc_grad_tau, per spin", "spin meta XC gradient launch"})
                      : tau_term ? (fused ? Form{"xc_grad_meta", "meta XC gradient launch (fused)"} : Form{"xc_grad + xc_grad_tau", "meta XC gradient launch"})
                      : spin   ? Form{"xc_grad_spin", fused ? "XC spin gradient launch (fused)" : "XC spin gradient launch"}
                               : Form{"xc_grad", "XC gradient launch"};
    ScopedTimer t(s, form.timer);
    const hipError_t e =
        tau_term && spin ? (fused ? launch_xc_grad_meta_spin_fused(s->stream, T, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), b.coef.d(), ct, ctb, Da, Db, slabs, out)
                                  : launch_xc_grad_meta_spin_plain(s->stream, G, T, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), b.coef.d(), ct, ctb, Da, Db, slabs, out))
        : tau_term ? (fused ? launch_xc_grad_meta_fused(s->stream, T, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), ct, Da, slabs, out)
                          : launch_xc_grad_meta_plain(s->stream, G, T, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), ct, Da, slabs, out))
        : spin   ? (fused ? launch_xc_grad_spin_fused(s->stream, G, gga, fac, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), b.coef.d(), Da, Db, slabs, out)
                          : launch_xc_grad_spin(s->stream, G, gga, fac, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), b.coef.d(), Da, Db, slabs, out))
                 : launch_xc_grad(s->stream, G, gga, fac, ngrid, nao, ao, ao_grad, ao_hess, a.coef.d(), Da, slabs, out);
    return hip_ok(s, e, form.what);
}

// The energy per volume of the functional at the density of the call -- DFT_ComputeXCEnergyDensity, its open-shell
// counterpart (DFT_ComputeXCSpin's refusal) and the meta-GGA's, at the density and tau of dm: the density stage above, then
// the body of the entry's pointwise kernel with unit weight (k_xc_edens, the spin-resolved body, k_xc_edens_meta,
// k_xc_edens_meta_spin).  Nothing
// here reads the padded matrix but k_tau.  Never the one-kernel plan, never recorded; asynchronous on the solver's stream.
bool xc_energy_density(XCSolver *s, const XcgEntry &E, long ngrid, int nao, const double *const dm[2], const double *ao, const double *ao_grad,
                       double *e_out)
{
    if (!xcg_enter(s, E, false, ngrid, nao, dm, ao, nullptr, ao_grad, nullptr, e_out) || !device_ready(s)) return false;
    const bool gga = s->needs_grad;
    const SweepPlan P = plan_sweep(s, ngrid, nao, ao, gga ? ao_grad : nullptr, false);
    if (!reserve_xcg(s, E, P, ngrid, WS_GRAD | WS_SIGMA, 0) || !xcg_density(s, E, P, E.meta, ngrid, nao, dm, ao, ao_grad)) return false;
    const Planes &a = s->xcg[0], &b = s->xcg[1];
    ScopedTimer t(s, E.timer);
    const hipError_t e =
        E.meta && E.nspin == 2 ? launch_xc_edens_meta_spin(s->stream, s->mix.c, s->meta, ngrid, a.rho.d(), b.rho.d(), a.grad.d(), b.grad.d(),
                                                           s->xcg_tau.d(), s->xcg_tau.d() + (size_t)ngrid, e_out)
        : E.meta       ? launch_xc_edens_meta(s->stream, s->mix.c, s->meta, ngrid, a.rho.d(), a.grad.d(), s->xcg_tau.d(), e_out)
        : E.nspin == 2 ? launch_xc_edens_spin(s->stream, xc_type_index(s), gga, s->mix.c, ngrid, a.rho.d(), b.rho.d(), gga ? a.grad.d() : nullptr,
                                              gga ? b.grad.d() : nullptr, e_out)
                       : launch_xc_edens(s->stream, xc_type_index(s), gga, s->mix.c, s->quirks, ngrid, a.rho.d(), a.sigma.d(), a.grad.d(), e_out);
    return hip_ok(s, e, E.launch);
}

// sum_g f_g D_B cell_g (DFT_BeckeWeightGradient, becke.hip).  The tables a_CD = clamp((rad_D / rad_C - rad_C / rad_D) / 4,
// +-1/2) with rad = sqrt(radius) + 1e-200 (grid_gen.becke_weights, operation for operation) and 1 / R_CD are made here and
// kept on the device until the atoms change; only then does the call wait for the stream.
bool becke_weight_gradient(XCSolver *s, long ngrid, int natm, const double *atom_xyz, const double *atom_radius, const double *coords,
                           const int *owner, const double *f, double *cell_out, double *out)
{
    s->last_error.clear();
    s->n_timed = 0;
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return false; }
    if (ngrid <= 0 || natm <= 0) { set_error(s, "DFT_BeckeWeightGradient: bad sizes ngrid=%ld natm=%d", ngrid, natm); return false; }
    if (!atom_xyz || !atom_radius || !coords || !owner || !f || !out) {
        set_error(s, "DFT_BeckeWeightGradient needs the atom positions and radii, the coordinates, the owners, f and the output");
        return false;
    }
    const BeckePlan B = becke_plan(s->num_cu, ngrid, natm);
    if (B.lds > BECKE_LDS_MAX) {
        set_error(s, "DFT_BeckeWeightGradient: natm=%d needs %zu bytes of LDS per workgroup for a tile of %d points, above the %zu a "
                     "workgroup has; distant atoms are not screened", natm, B.lds, B.tp, BECKE_LDS_MAX);
        return false;
    }
    const size_t n2 = (size_t)natm * natm;
    std::vector<double> tab(3 * (size_t)natm + 2 * n2);
    double *xyz = tab.data(), *at = xyz + 3 * natm, *rt = at + n2;
    std::vector<double> rad(natm);
    for (int i = 0; i < natm; ++i) {
        if (!(atom_radius[i] > 0.0) || !std::isfinite(atom_radius[i])) {
            set_error(s, "DFT_BeckeWeightGradient: radius %g of atom %d is not positive", atom_radius[i], i);
            return false;
        }
        rad[i] = std::sqrt(atom_radius[i]) + 1e-200;
        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = atom_xyz[3 * i + k];
    }
    for (int i = 0; i < natm; ++i)
        for (int j = 0; j < natm; ++j) {
            const double a = 0.25 * (rad[j] / rad[i] - rad[i] / rad[j]);
            at[(size_t)i * natm + j] = std::min(0.5, std::max(-0.5, a));
            const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
            const double R = std::sqrt(dx * dx + dy * dy + dz * dz);
            if (i != j && !(R > 0.0 && std::isfinite(R))) {
                set_error(s, "DFT_BeckeWeightGradient: atoms %d and %d coincide (or a position is not finite)", i, j);
                return false;
            }
            rt[(size_t)i * natm + j] = i == j ? 1.0 : 1.0 / R;
        }
    if (!reserve(s, s->becke_slabs, sizeof(double) * (size_t)B.nwg * 3 * natm, "hipMalloc(Becke slabs)", false)) return false;
    if (tab != s->becke_tab_host) {
        s->becke_tab_host.clear();
        if (!reserve(s, s->becke_tab, sizeof(double) * tab.size(), "hipMalloc(Becke tables)", false) ||
            !hip_ok(s, hipMemcpyAsync(s->becke_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s->stream), "upload Becke tables") ||
            !hip_ok(s, hipStreamSynchronize(s->stream), "synchronise"))
            return false;
        s->becke_tab_host.swap(tab);
    }
    const double *d_xyz = s->becke_tab.d(), *d_at = d_xyz + 3 * natm, *d_rt = d_at + n2;
    ScopedTimer t(s, "becke_wgrad");
    return hip_ok(s, launch_becke_wgrad(s->stream, B, ngrid, natm, d_xyz, d_at, d_rt, coords, owner, f, cell_out, s->becke_slabs.d(), out),
                  "Becke weight gradient launch");
}

} // namespace

extern "C" {

int DFT_GetVersion(void) { return 5; }   // 4: DFT_CreateSolverMix / DFT_GetMix; 5: DFT_PointCoulomb*

// Option "publish": does this runtime perform a stream memory write on a pinned, host-mapped word?  Asked once, with an
// ordinary call on the stream a new solver uses (the null stream); any error code, or a value that did not arrive, leaves
// the kernel path in place.
static void probe_publish(XCSolver *s)
{
    if (!s->h_exc_dev) return;
    if (hipHostMalloc((void **)&s->h_seq, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&s->h_seq_dev, s->h_seq, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (s->h_seq) (void)hipHostFree(s->h_seq);
        s->h_seq = s->h_seq_dev = nullptr;
        return;
    }
    *s->h_seq = 0;
    s->seq = 1;
    if (hipStreamWriteValue64(s->stream, s->h_seq_dev, s->seq, 0) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    s->publish_ok = *(volatile unsigned long long *)s->h_seq == s->seq;
}

static XCSolver *create_solver(int type, const double *mix)
{
    XCSolver *s = new (std::nothrow) XCSolver();
    if (!s) return nullptr;
    s->type = type;
    s->needs_grad = type != SOLVER_LDA;
    if (const char *e = getenv("QCDFT_DM_FACTOR")) s->dm_factor = !strcmp(e, "1");   // sampled here, once
    if (mix) {
        s->needs_grad = false;
        for (int k = 0; k < XC_NCOMP; ++k) {
            s->mix.c[k] = mix[k];
            if (k >= XC_PBE_X && mix[k] != 0.0) s->needs_grad = true;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            s->device_ok = true;
            s->device = dev;
            s->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
        if (s->device_ok) {
            if (hipHostMalloc((void **)&s->h_exc, sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                hipHostGetDevicePointer((void **)&s->h_exc_dev, s->h_exc, 0) != hipSuccess) {
                (void)hipGetLastError();
                s->h_exc = nullptr;
                s->h_exc_dev = nullptr;
            }
            probe_publish(s);
        }
    } else {
        (void)hipGetLastError();
        s->last_error = "no usable HIP device";
    }
    return s;
}

XCSolver *DFT_CreateSolver(int type)
{
    if (type != SOLVER_LDA && type != SOLVER_GGA && type != SOLVER_B3LYP) return nullptr;   // SOLVER_MIX needs weights
    return create_solver(type, nullptr);
}

XCSolver *DFT_CreateSolverMix(const double *weights, int ncomp)
{
    if (!weights || ncomp != XC_NCOMP) return nullptr;
    bool any = false;
    for (int k = 0; k < XC_NCOMP; ++k) {
        if (!std::isfinite(weights[k])) return nullptr;
        any = any || weights[k] != 0.0;
    }
    if (!any) return nullptr;
    return create_solver(SOLVER_MIX, weights);
}

XCSolver *DFT_CreateSolverMeta(const double *weights, int ncomp, const double *meta_weights, int nmeta)
{
    if (!weights || ncomp != XC_NCOMP || !meta_weights || nmeta != XC_NMETA) return nullptr;
    bool any = false;
    for (int k = 0; k < XC_NCOMP; ++k) {
        if (!std::isfinite(weights[k])) return nullptr;
        any = any || weights[k] != 0.0;
    }
    for (int k = 0; k < XC_NMETA; ++k) {
        if (!std::isfinite(meta_weights[k])) return nullptr;
        any = any || meta_weights[k] != 0.0;
    }
    if (!any) return nullptr;
    XCSolver *s = create_solver(SOLVER_MIX, weights);
    if (!s) return nullptr;
    s->is_meta = true;
    s->needs_grad = true;   // tau is made of the gradient planes: always the four-plane form
    for (int k = 0; k < XC_NMETA; ++k) {
        s->meta[k] = meta_weights[k];
        s->meta_active = s->meta_active || meta_weights[k] != 0.0;
    }
    return s;
}

int DFT_GetMeta(XCSolver *s, double *meta_weights_out, int nmeta)
{
    if (!s || !meta_weights_out || nmeta != XC_NMETA) return -1;
    for (int k = 0; k < XC_NMETA; ++k) meta_weights_out[k] = s->meta[k];
    return 0;
}

int DFT_GetMix(XCSolver *s, double *weights_out, int ncomp)
{
    if (!s || !weights_out || ncomp != XC_NCOMP) return -1;
    for (int k = 0; k < XC_NCOMP; ++k) weights_out[k] = 0.0;
    switch (s->type) {
    case SOLVER_LDA: weights_out[XC_SLATER_X] = 1.0; weights_out[XC_VWN5_C] = 1.0; break;
    case SOLVER_GGA: weights_out[XC_PBE_X] = 1.0; weights_out[XC_PBE_C] = 1.0; break;
    case SOLVER_B3LYP:   // the mixing of xc::b3lyp_point
        weights_out[XC_SLATER_X] = 0.80; weights_out[XC_B88_X] = 0.72; weights_out[XC_VWN_RPA_C] = 0.19; weights_out[XC_LYP_C] = 0.81;
        break;
    default:
        for (int k = 0; k < XC_NCOMP; ++k) weights_out[k] = s->mix.c[k];
    }
    return 0;
}

void DFT_DestroySolver(XCSolver *s)
{
    if (!s) return;
    DeviceGuard dg(s);   // in scope until the solver is deleted: its buffers free themselves on its device
    if (s->device_ok) {
        (void)hipStreamSynchronize(s->stream);
        drop_graphs(s);
        if (s->cap_stream) (void)hipStreamDestroy(s->cap_stream);
        if (s->h_exc) (void)hipHostFree(s->h_exc);
        if (s->h_seq) (void)hipHostFree(s->h_seq);
        for (Timing &t : s->timings) {
            (void)hipEventDestroy(t.t0);
            (void)hipEventDestroy(t.t1);
        }
    }
    delete s;
}

// Option "graph": the launches of a synchronous call, recorded once per (pointers, sizes) and replayed as one HIP graph.
constexpr double GRAPH_AUTO_ELEMS = 2.0e6;

static SweepGraph *find_sweep(XCSolver *s, const SweepArgs &a)
{
    for (SweepGraph &g : s->graphs)
        if (g.key == a) return &g;
    return nullptr;
}

// Records the sweep for `a` on the solver's recording stream; on any failure the key is marked and runs as plain launches.
static bool record_sweep(XCSolver *s, const SweepArgs &a)
{
    if (!s->cap_stream && hipStreamCreateWithFlags(&s->cap_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const unsigned long gen = s->graph_gen;
    if (hipStreamBeginCapture(s->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    hipStream_t user = s->stream;
    s->stream = s->cap_stream;
    s->recording = true;   // replay keeps the publishing kernel: stream memory operations are not recorded
    const bool ok = xc_sweep(s, a.ngrid, a.nao, a.dm, a.ao, a.grad, a.w, a.vxc, true, a.cocc, a.nocc);
    s->recording = false;
    s->stream = user;
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(s->cap_stream, &graph);
    hipGraphExec_t exec = nullptr;
    const bool good = ok && e == hipSuccess && graph && gen == s->graph_gen &&
                      hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (!good) (void)hipGetLastError();
    SweepGraph *g = gen == s->graph_gen ? find_sweep(s, a) : nullptr;
    if (!g) {
        if (exec) (void)hipGraphExecDestroy(exec);
        return false;
    }
    g->exec = good ? exec : nullptr;
    g->bad = !good;
    return good;
}

// True when the call was submitted as a recorded graph (recording it first if this is the key's second call).
static bool replay_sweep(XCSolver *s, const SweepArgs &a)
{
    SweepGraph *g = find_sweep(s, a);
    if (!g || g->bad) return false;
    if (!g->exec && !record_sweep(s, a)) return false;
    g = find_sweep(s, a);
    if (!g || !g->exec) return false;
    if (hipGraphLaunch(g->exec, s->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphExecDestroy(g->exec);
        g->exec = nullptr;
        g->bad = true;
        return false;
    }
    g->stamp = ++s->graph_clock;
    s->last_error.clear();
    return true;
}

// After a successful call: remember the key (at most eight, least recently used out first).
static void note_sweep(XCSolver *s, const SweepArgs &a)
{
    if (SweepGraph *g = find_sweep(s, a)) {
        ++g->seen;
        g->stamp = ++s->graph_clock;
        return;
    }
    if (s->graphs.size() >= 8) {
        size_t old = 0;
        for (size_t i = 1; i < s->graphs.size(); ++i)
            if (s->graphs[i].stamp < s->graphs[old].stamp) old = i;
        if (s->graphs[old].exec) (void)hipGraphExecDestroy(s->graphs[old].exec);
        s->graphs.erase(s->graphs.begin() + (long)old);
    }
    SweepGraph g;
    g.key = a;
    g.seen = 1;
    g.stamp = ++s->graph_clock;
    s->graphs.push_back(g);
}

// The synchronous call: sweep + wait for Exc (shared by DFT_ComputeXC / DFT_ComputeXC64 / DFT_ComputeXCOcc)
static double xc_call_sync(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm,
                           unsigned long long d_ao, unsigned long long d_ao_grad,
                           unsigned long long d_w, unsigned long long d_vxc,
                           unsigned long long d_cocc, int nocc)
{
    if (!s) return 0.0;
    DeviceGuard dg(s);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (s->h_exc) *s->h_exc = nan; // before anything is enqueued: the last kernel overwrites it
    SweepArgs a{(long)ngrid, nao, nocc, (const double *)d_dm, (const double *)d_ao, (const double *)d_ao_grad,
                (const double *)d_w, (double *)d_vxc, (const double *)d_cocc};
    // Option "dm_factor": a caller that holds dm alone.  The factor of dm stands in for the occupied orbitals where occ_pays
    // takes the occupied form for its rank; a dm that does not factorise, or a rank at which the dm kernels do fewer
    // MFMAs, leaves the call exactly as it is without the option.
    const bool dmf = s->dm_factor && d_dm && !d_cocc;
    s->used_dm_factor = 0;
    s->timed_base = 0;
    if (dmf) {
        s->dm_factor_rank = 0;
        s->n_timed = 0;
        if (s->device_ok && occ_allowed(s) && ngrid > 0 && nao > 0 && !takes_tiny(s, (long)ngrid, nao) &&
            reserve(s, s->dmf_c, sizeof(double) * (size_t)nao * std::max(nao / 2, 1), "hipMalloc(dm factor, packed)")) {
            const int rank = factor_density(s, nao, a.dm, 0, 0.0, (double *)s->dmf_c.p, nullptr);
            if (rank > 0) {
                s->dm_factor_rank = rank;
                OccPlan pl;
                if (occ_pays(s, nao, rank, pl)) {
                    a.cocc = (const double *)s->dmf_c.p;
                    a.nocc = nocc = rank;
                    s->used_dm_factor = 1;
                }
            }
            s->timed_base = s->n_timed;   // with "profile": the factor kernels stay in front of the sweep's
        }
    }
    const bool graphed = !dmf && !s->profile && s->h_exc_dev && ngrid > 0 && nao > 0 &&
                         (s->graph > 0 || (s->graph < 0 && (double)ngrid * nao <= GRAPH_AUTO_ELEMS));
    if (graphed && replay_sweep(s, a)) s->wait_mode = 0; // a recorded sweep ends with the publishing kernel
    else if (!xc_sweep(s, a.ngrid, nao, a.dm, a.ao, a.grad, a.w, a.vxc, true, a.cocc, nocc))
        return nan;
    if (graphed) note_sweep(s, a);
    s->used_publish = s->wait_mode == 1;
    if (s->h_exc_dev) { // Exc is written into host-mapped memory by the call's last kernel
        volatile double *hx = s->h_exc;
        if (s->spin_wait && s->wait_mode == 1) {
            // Option "publish": the completion word is this call's sequence number, stored by a stream memory write that
            // the runtime performs after every earlier command of the stream -- the reduce kernel, whose finishing block
            // left Exc in *hx, included.  The same bounded spin, the same meaning ("the whole call has completed"); a
            // faulted stream ends it, and the stream is then polled to completion as below.
            volatile unsigned long long *hs = s->h_seq;
            const unsigned long long want = s->seq;
            for (unsigned spins = 1; *hs != want; ++spins) {
                if ((spins & 0xFFF) == 0 && hipStreamQuery(s->stream) != hipErrorNotReady) break;
                __builtin_ia32_pause();
            }
            __atomic_thread_fence(__ATOMIC_ACQUIRE); // Exc is read after the sequence word
            if (s->strict_sync || *hs != want || std::isnan(*hx)) {
                hipError_t q;
                while ((q = hipStreamQuery(s->stream)) == hipErrorNotReady) __builtin_ia32_pause();
                if (!hip_ok(s, q, "XC sweep")) return nan;
            }
        } else if (s->spin_wait && s->wait_mode == 0) {
            // The word is stored by the call's LAST kernel.  Default: that is the one-block k_finish_exc, which stream
            // order starts only after the Vxc reduce (and everything before it) has completed -- seeing the word means
            // the whole call is done, for consumers on any stream and for host reads, the reference's contract
            // (blocking 8-byte copy + cudaFree, dft_solver.cu:575-582).  With option "fuse_finish" = 1 the reduce
            // kernel's highest-index block stores it (no finishing launch): then it only orders consumers on the
            // SOLVER'S stream (the reference's pattern, d_vxc.get() on the null stream, dft.py:211), and
            // "strict_sync" = 1 adds a poll of the stream to completion for the others.  Both spins are bounded by
            // the stream state: a faulted kernel or an Exc that really is NaN ends them.
            for (unsigned spins = 1; std::isnan(*hx); ++spins) {
                if ((spins & 0xFFF) == 0 && hipStreamQuery(s->stream) != hipErrorNotReady) break;
                __builtin_ia32_pause();
            }
            if (s->strict_sync || std::isnan(*hx)) {
                hipError_t q;
                while ((q = hipStreamQuery(s->stream)) == hipErrorNotReady) __builtin_ia32_pause();
                if (!hip_ok(s, q, "XC sweep")) return nan;
            }
        } else if (!hip_ok(s, hipStreamSynchronize(s->stream), "synchronise")) {
            return nan;
        }
        const double out = *hx;
        if (std::isnan(out)) set_error(s, "Exc is NaN after the sweep completed (non-finite inputs, or the finishing kernel did not run)");
        return out;
    }
    double out = nan;
    if (!hip_ok(s, hipMemcpyAsync(&out, s->exc.p, sizeof(double), hipMemcpyDeviceToHost, s->stream), "copy Exc") ||
        !hip_ok(s, hipStreamSynchronize(s->stream), "synchronise"))
        return nan;
    if (std::isnan(out)) set_error(s, "Exc is NaN after the sweep completed (non-finite inputs)");
    return out;
}

double DFT_ComputeXC64(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm,
                       unsigned long long d_ao, unsigned long long d_ao_grad,
                       unsigned long long d_w, unsigned long long d_vxc)
{
    return xc_call_sync(s, ngrid, nao, d_dm, d_ao, d_ao_grad, d_w, d_vxc, 0ULL, 0);
}

double DFT_ComputeXCOcc(XCSolver *s, long long ngrid, int nao, int nocc, unsigned long long d_cocc,
                        unsigned long long d_dm, unsigned long long d_ao, unsigned long long d_ao_grad,
                        unsigned long long d_w, unsigned long long d_vxc)
{
    if (s && !d_cocc) {
        set_error(s, "DFT_ComputeXCOcc needs the occupied orbitals");
        return std::numeric_limits<double>::quiet_NaN();
    }
    return xc_call_sync(s, ngrid, nao, d_dm, d_ao, d_ao_grad, d_w, d_vxc, d_cocc, nocc);
}

int DFT_ComputeXCOccAsync(XCSolver *s, long long ngrid, int nao, int nocc, unsigned long long d_cocc,
                          unsigned long long d_dm, unsigned long long d_ao, unsigned long long d_ao_grad,
                          unsigned long long d_w, unsigned long long d_vxc, unsigned long long d_exc)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    if (!d_cocc) { set_error(s, "DFT_ComputeXCOccAsync needs the occupied orbitals"); return -1; }
    if (!xc_sweep(s, (long)ngrid, nao, (const double *)d_dm, (const double *)d_ao,
                  (const double *)d_ao_grad, (const double *)d_w, (double *)d_vxc, false, (const double *)d_cocc, nocc, (double *)d_exc))
        return -1;
    return 0;
}

double DFT_ComputeXC(XCSolver *s, int ngrid, int nao, unsigned long long d_dm,
                     unsigned long long d_ao, unsigned long long d_ao_grad,
                     unsigned long long d_w, unsigned long long d_vxc)
{
    return DFT_ComputeXC64(s, ngrid, nao, d_dm, d_ao, d_ao_grad, d_w, d_vxc);
}

int DFT_ComputeXCAsync(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm,
                       unsigned long long d_ao, unsigned long long d_ao_grad,
                       unsigned long long d_w, unsigned long long d_vxc,
                       unsigned long long d_exc)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    if (!xc_sweep(s, (long)ngrid, nao, (const double *)d_dm, (const double *)d_ao,
                  (const double *)d_ao_grad, (const double *)d_w, (double *)d_vxc, false, nullptr, 0, (double *)d_exc))
        return -1;
    return 0;
}

int DFT_FxcPrepare(XCSolver *s, long long ngrid, int nao, int nocc, unsigned long long d_cocc, unsigned long long d_dm0,
                   unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_weights)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return fxc_prepare(s, (long)ngrid, nao, nocc, (const double *)d_cocc, (const double *)d_dm0, (const double *)d_ao,
                       (const double *)d_ao_grad, (const double *)d_weights) ? 0 : -1;
}

int DFT_FxcPrepareSpin(XCSolver *s, long long ngrid, int nao, int nocc, unsigned long long d_cocc, unsigned long long d_dm0,
                       unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_weights, int kind)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    if (kind != 1 && kind != 2) {
        s->last_error.clear();
        set_error(s, "DFT_FxcPrepareSpin: unknown kind %d (1 triplet, 2 singlet through the spin-resolved bodies)", kind);
        return -1;
    }
    return fxc_prepare(s, (long)ngrid, nao, nocc, (const double *)d_cocc, (const double *)d_dm0, (const double *)d_ao,
                       (const double *)d_ao_grad, (const double *)d_weights, kind) ? 0 : -1;
}

int DFT_FxcApplyKind(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm1, unsigned long long d_ao,
                     unsigned long long d_ao_grad, unsigned long long d_v1, int kind)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return fxc_apply(s, (long)ngrid, nao, (const double *)d_dm1, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_v1, kind) ? 0 : -1;
}

int DFT_FxcApply(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm1, unsigned long long d_ao,
                 unsigned long long d_ao_grad, unsigned long long d_v1)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return fxc_apply(s, (long)ngrid, nao, (const double *)d_dm1, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_v1) ? 0 : -1;
}

int DFT_FxcPrepareSpinPol(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm0_a, unsigned long long d_dm0_b,
                          unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_weights)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return fxc_prepare_spinpol(s, (long)ngrid, nao, (const double *)d_dm0_a, (const double *)d_dm0_b, (const double *)d_ao,
                               (const double *)d_ao_grad, (const double *)d_weights) ? 0 : -1;
}

int DFT_FxcApplySpinPol(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm1_a, unsigned long long d_dm1_b,
                        unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_v1_a, unsigned long long d_v1_b)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return fxc_apply_spinpol(s, (long)ngrid, nao, (const double *)d_dm1_a, (const double *)d_dm1_b, (const double *)d_ao,
                             (const double *)d_ao_grad, (double *)d_v1_a, (double *)d_v1_b) ? 0 : -1;
}

int DFT_FxcSpinPolTable(XCSolver *s, unsigned long long d_out, long long max_doubles)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    if (!fxc_slot_ok(s, s->fxc_pol, "DFT_FxcSpinPolTable", "DFT_FxcPrepareSpinPol", "", 0, 0)) return -1;
    const int planes = fxc_pol_planes(s->needs_grad);
    const long long need = (long long)planes * s->fxc_pol.ngrid;
    if (!d_out || max_doubles < need) { set_error(s, "DFT_FxcSpinPolTable needs room for %lld doubles", need); return -1; }
    if (!hip_ok(s, hipMemcpyAsync((void *)d_out, s->fxc_pol.table.p, sizeof(double) * (size_t)need, hipMemcpyDeviceToDevice, s->stream), "copy table"))
        return -1;
    return planes;
}

int DFT_ComputeXCSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                      unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_w,
                      unsigned long long d_vxc_a, unsigned long long d_vxc_b, double *exc)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const SyncEntry E{"DFT_ComputeXCSpin",
                             "DFT_ComputeXCSpin needs both density matrices, the AO values, the grid weights, both output matrices and exc",
                             "spin sweep", "hipMalloc(spin exc)", "spin pointwise launch", 2, false, false};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    double *const vxc[2] = {(double *)d_vxc_a, (double *)d_vxc_b};
    return xc_sweep_sync(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (const double *)d_w, vxc, exc) ? 0 : -1;
}

int DFT_ComputeTau(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao_grad, unsigned long long d_tau)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    s->n_timed = 0;
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (ngrid <= 0 || nao <= 0) { set_error(s, "bad sizes ngrid=%lld nao=%d", ngrid, nao); return -1; }
    if (!d_dm || !d_ao_grad || !d_tau) { set_error(s, "DFT_ComputeTau needs the density matrix, ao_grad and the output"); return -1; }
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    double *const tau[2] = {(double *)d_tau, nullptr};
    return compute_tau(s, 1, (long)ngrid, nao, dm, (const double *)d_ao_grad, tau) ? 0 : -1;
}

int DFT_ComputeXCMeta(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao, unsigned long long d_w,
                      unsigned long long d_ao_grad, unsigned long long d_vxc, double *exc)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const SyncEntry E{"DFT_ComputeXCMeta",
                             "DFT_ComputeXCMeta needs the density matrix, the AO values, the grid weights, the output matrix and exc",
                             "meta-GGA sweep", "hipMalloc(meta exc)", "meta pointwise launch", 1, true, false};
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    double *const vxc[2] = {(double *)d_vxc, nullptr};
    return xc_sweep_sync(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (const double *)d_w, vxc, exc) ? 0 : -1;
}

int DFT_ComputeTauSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                       unsigned long long d_ao_grad, unsigned long long d_tau_a, unsigned long long d_tau_b)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    s->n_timed = 0;
    if (ngrid <= 0 || nao <= 0) { set_error(s, "bad sizes ngrid=%lld nao=%d", ngrid, nao); return -1; }
    if (!d_dm_a || !d_dm_b || !d_ao_grad || !d_tau_a || !d_tau_b) {
        set_error(s, "DFT_ComputeTauSpin needs both density matrices, ao_grad and both outputs: a pointer is null");
        return -1;
    }
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    double *const tau[2] = {(double *)d_tau_a, (double *)d_tau_b};
    return compute_tau(s, 2, (long)ngrid, nao, dm, (const double *)d_ao_grad, tau) ? 0 : -1;
}

int DFT_ComputeXCMetaSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                          unsigned long long d_ao, unsigned long long d_w, unsigned long long d_ao_grad,
                          unsigned long long d_vxc_a, unsigned long long d_vxc_b, double *exc)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const SyncEntry E{"DFT_ComputeXCMetaSpin",
                             "DFT_ComputeXCMetaSpin needs both density matrices, the AO values, the grid weights, ao_grad (tau is made of the "
                             "gradient planes), both output matrices and exc: a pointer is null",
                             "spin-resolved meta-GGA sweep", "hipMalloc(spin meta exc)", "spin meta pointwise launch", 2, true, true};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    double *const vxc[2] = {(double *)d_vxc_a, (double *)d_vxc_b};
    return xc_sweep_sync(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (const double *)d_w, vxc, exc) ? 0 : -1;
}

void DFT_ComputeCoulomb(XCSolver *s, int nao, unsigned long long d_eri, unsigned long long d_dm,
                        unsigned long long d_J)
{
    if (!s) return;
    DeviceGuard dg(s);
    jk(s, nao, (const double *)d_eri, (const double *)d_dm, (double *)d_J, nullptr);
}

void DFT_ComputeExchange(XCSolver *s, int nao, unsigned long long d_eri, unsigned long long d_dm,
                         unsigned long long d_K)
{
    if (!s) return;
    DeviceGuard dg(s);
    jk(s, nao, (const double *)d_eri, (const double *)d_dm, nullptr, (double *)d_K);
}

void DFT_ComputeJK(XCSolver *s, int nao, unsigned long long d_eri, unsigned long long d_dm,
                   unsigned long long d_J, unsigned long long d_K)
{
    if (!s) return;
    DeviceGuard dg(s);
    jk(s, nao, (const double *)d_eri, (const double *)d_dm, (double *)d_J, (double *)d_K);
}

int DFT_ComputeJKRows(XCSolver *s, int nao, int i_lo, int i_hi, unsigned long long d_eri_rows,
                      unsigned long long d_dm, unsigned long long d_J, unsigned long long d_K)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    jk(s, nao, (const double *)d_eri_rows, (const double *)d_dm, (double *)d_J, (double *)d_K, i_lo, i_hi - i_lo);
    return s->last_error.empty() ? 0 : -1;
}

int DFT_ComputeJKFactorized(XCSolver *s, int nao, int naux, int nocc, unsigned long long d_chol,
                            unsigned long long d_dm, unsigned long long d_cocc, unsigned long long d_J,
                            unsigned long long d_K)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->n_timed = 0;
    return jk_factorized(s, nao, naux, nocc, (const double *)d_chol, (const double *)d_dm,
                         (const double *)d_cocc, (double *)d_J, (double *)d_K);
}

int DFT_ComputeJKFactorizedResponse(XCSolver *s, int nao, int naux, int nocc, int nvec, unsigned long long d_chol,
                                    unsigned long long d_a, unsigned long long d_b, unsigned long long d_J,
                                    unsigned long long d_M)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->n_timed = 0;
    return jk_factorized_response(s, nao, naux, nocc, nvec, (const double *)d_chol, (const double *)d_a,
                                  (const double *)d_b, (double *)d_J, (double *)d_M);
}

int DFT_FactorDensity(XCSolver *s, int nao, unsigned long long d_dm, int max_rank, double tol,
                      unsigned long long d_cocc_out, double *info4)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->n_timed = 0;
    return factor_density(s, nao, (const double *)d_dm, max_rank, tol, (double *)d_cocc_out, info4);
}

int DFT_EvalAO(XCSolver *s, long long ngrid, int nao, int nshell, const double *shl_xyz,
               const int *shl_l, const int *shl_nprim, const int *shl_off, const int *shl_ao,
               const double *prim_exp, const double *prim_coef, int nprim_total,
               unsigned long long d_coords, unsigned long long d_ao, unsigned long long d_ao_grad)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    s->n_timed = 0;
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (ngrid <= 0) { set_error(s, "bad AO sizes"); return -1; }
    AoTable tab;
    if (!prepare_ao_table(s, nao, nshell, shl_xyz, shl_l, shl_nprim, shl_off, shl_ao, prim_exp, prim_coef, nprim_total, tab)) return -1;
    ScopedTimer t(s, "eval_ao");
    launch_ao(s, tab, (long)ngrid, nao, (const double *)d_coords, (double *)d_ao, (double *)d_ao_grad);
    return hip_ok(s, hipGetLastError(), "AO launch") ? 0 : -1;
}

int DFT_EvalAOHess(XCSolver *s, long long ngrid, int nao, int nshell, const double *shl_xyz,
                   const int *shl_l, const int *shl_nprim, const int *shl_off, const int *shl_ao,
                   const double *prim_exp, const double *prim_coef, int nprim_total,
                   unsigned long long d_coords, unsigned long long d_hess)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    s->n_timed = 0;
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (ngrid <= 0) { set_error(s, "bad AO sizes"); return -1; }
    if (!d_coords || !d_hess) { set_error(s, "DFT_EvalAOHess needs the coordinates and the output planes"); return -1; }
    AoTable tab;
    if (!prepare_ao_table(s, nao, nshell, shl_xyz, shl_l, shl_nprim, shl_off, shl_ao, prim_exp, prim_coef, nprim_total, tab)) return -1;
    ScopedTimer t(s, "eval_ao_hess");
    return hip_ok(s, launch_eval_ao_hess(s->stream, (long)ngrid, nao, tab.nchunk, tab.maxcol, tab.sh, tab.exp, tab.coef, tab.chunks,
                                         (const double *)d_coords, (double *)d_hess), "AO Hessian launch") ? 0 : -1;
}

int DFT_ComputeXCGradient(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao,
                          unsigned long long d_weights, unsigned long long d_ao_grad, unsigned long long d_ao_hess,
                          unsigned long long d_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCGradient", "DFT_ComputeXCGradient needs dm, the AO values, the grid weights and the output",
                            "hipMalloc(Dsym)", "hipMalloc(gradient slabs)", "XC gradient density launch", "XC gradient pointwise launch",
                            "xc_points", 1, false};
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    return xc_gradient(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_weights, (const double *)d_ao_grad,
                       (const double *)d_ao_hess, (double *)d_out) ? 0 : -1;
}

int DFT_ComputeXCGradientSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                              unsigned long long d_ao, unsigned long long d_weights, unsigned long long d_ao_grad,
                              unsigned long long d_ao_hess, unsigned long long d_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCGradientSpin",
                            "DFT_ComputeXCGradientSpin needs both density matrices, the AO values, the grid weights and the output",
                            "hipMalloc(Dsym of both spins)", "hipMalloc(spin gradient slabs)", "spin gradient: density launch",
                            "spin pointwise launch", "xc_points_spin", 2, false};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    return xc_gradient(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_weights, (const double *)d_ao_grad,
                       (const double *)d_ao_hess, (double *)d_out) ? 0 : -1;
}

int DFT_ComputeXCGradientMeta(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao,
                              unsigned long long d_weights, unsigned long long d_ao_grad, unsigned long long d_ao_hess,
                              unsigned long long d_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCGradientMeta",
                            "DFT_ComputeXCGradientMeta needs dm, the AO values, the grid weights, ao_grad (tau is made of the gradient planes), "
                            "ao_hess and the output: a pointer is null",
                            "hipMalloc(meta gradient Dsym)", "hipMalloc(meta gradient slabs)", "meta gradient: density launch",
                            "meta pointwise launch", "xc_points_meta", 1, true};
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    return xc_gradient(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_weights, (const double *)d_ao_grad,
                       (const double *)d_ao_hess, (double *)d_out) ? 0 : -1;
}

int DFT_ComputeXCGradientMetaSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                                  unsigned long long d_ao, unsigned long long d_weights, unsigned long long d_ao_grad,
                                  unsigned long long d_ao_hess, unsigned long long d_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCGradientMetaSpin",
                            "DFT_ComputeXCGradientMetaSpin needs both density matrices, the AO values, the grid weights, ao_grad (tau is made of "
                            "the gradient planes), ao_hess and the output: a pointer is null",
                            "hipMalloc(meta gradient Dsym of both spins)", "hipMalloc(spin meta gradient slabs)",
                            "spin meta gradient: density launch", "spin meta pointwise launch", "xc_points_meta_spin", 2, true};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    return xc_gradient(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_weights, (const double *)d_ao_grad,
                       (const double *)d_ao_hess, (double *)d_out) ? 0 : -1;
}

int DFT_ComputeXCEnergyDensity(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao,
                               unsigned long long d_ao_grad, unsigned long long d_e_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCEnergyDensity", "DFT_ComputeXCEnergyDensity needs dm, the AO values and the output",
                            "hipMalloc(Dsym)", nullptr, "energy density: density launch", "energy density launch", "xc_edens", 1, false};
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    return xc_energy_density(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_e_out) ? 0 : -1;
}

int DFT_ComputeXCEnergyDensitySpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                                   unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_e_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCEnergyDensitySpin",
                            "DFT_ComputeXCEnergyDensitySpin needs both density matrices, the AO values and the output",
                            "hipMalloc(Dsym of both spins)", nullptr, "spin energy density: density launch", "spin energy density launch",
                            "xc_edens_spin", 2, false};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    return xc_energy_density(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_e_out) ? 0 : -1;
}

int DFT_ComputeXCEnergyDensityMeta(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm, unsigned long long d_ao,
                                   unsigned long long d_ao_grad, unsigned long long d_e_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCEnergyDensityMeta",
                            "DFT_ComputeXCEnergyDensityMeta needs dm, the AO values, ao_grad (tau is made of the gradient planes) and the "
                            "output: a pointer is null",
                            "hipMalloc(meta gradient Dsym)", nullptr, "meta gradient: density launch", "meta energy density launch",
                            "xc_edens_meta", 1, true};
    const double *const dm[2] = {(const double *)d_dm, nullptr};
    return xc_energy_density(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_e_out) ? 0 : -1;
}

int DFT_ComputeXCEnergyDensityMetaSpin(XCSolver *s, long long ngrid, int nao, unsigned long long d_dm_a, unsigned long long d_dm_b,
                                       unsigned long long d_ao, unsigned long long d_ao_grad, unsigned long long d_e_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    static const XcgEntry E{"DFT_ComputeXCEnergyDensityMetaSpin",
                            "DFT_ComputeXCEnergyDensityMetaSpin needs both density matrices, the AO values, ao_grad (tau is made of the "
                            "gradient planes) and the output: a pointer is null",
                            "hipMalloc(meta gradient Dsym of both spins)", nullptr, "spin meta gradient: density launch",
                            "spin meta energy density launch", "xc_edens_meta_spin", 2, true};
    const double *const dm[2] = {(const double *)d_dm_a, (const double *)d_dm_b};
    return xc_energy_density(s, E, (long)ngrid, nao, dm, (const double *)d_ao, (const double *)d_ao_grad, (double *)d_e_out) ? 0 : -1;
}

int DFT_BeckeWeightGradient(XCSolver *s, long long ngrid, int natm, const double *atom_xyz, const double *atom_radius,
                            unsigned long long d_coords, unsigned long long d_owner, unsigned long long d_f,
                            unsigned long long d_cell_out, unsigned long long d_out)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    return becke_weight_gradient(s, (long)ngrid, natm, atom_xyz, atom_radius, (const double *)d_coords, (const int *)d_owner,
                                 (const double *)d_f, (double *)d_cell_out, (double *)d_out) ? 0 : -1;
}

int DFT_ComputeXCDirect(XCSolver *s, long long ngrid, int nao, int nshell, const double *shl_xyz,
                        const int *shl_l, const int *shl_nprim, const int *shl_off, const int *shl_ao,
                        const double *prim_exp, const double *prim_coef, int nprim_total,
                        unsigned long long d_coords, unsigned long long d_w, unsigned long long d_dm,
                        unsigned long long d_vxc, unsigned long long d_exc, long long chunk_points)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    s->last_error.clear();
    if (!s->device_ok) { set_error(s, "no usable HIP device"); return -1; }
    if (ngrid <= 0 || nao <= 0 || !d_coords || !d_w || !d_dm || !d_vxc) { set_error(s, "bad arguments to DFT_ComputeXCDirect"); return -1; }
    AoTable tab;
    if (!prepare_ao_table(s, nao, nshell, shl_xyz, shl_l, shl_nprim, shl_off, shl_ao, prim_exp, prim_coef, nprim_total, tab)) return -1;
    const bool gga = s->needs_grad;
    const int nplane = gga ? 4 : 1;
    // chunk: its planes stay within ~96 MB (they are written by the AO kernel and read twice right after: an
    // Infinity-Cache-sized working set), but never fewer than 64 sixteen-point tiles per CU; a multiple of 256
    long chunk = chunk_points > 0 ? (long)chunk_points : std::max<long>((long)(96.0e6 / (8.0 * nao * nplane)), 1024L * s->num_cu);
    chunk = std::min<long>(((chunk + 255) / 256) * 256, (long)ngrid);
    const size_t plane = (size_t)chunk * nao;
    if (!reserve(s, s->ao_ws, sizeof(double) * plane * nplane, "hipMalloc(AO chunk)") ||
        !reserve(s, s->vtmp, sizeof(double) * ((size_t)nao * nao + 1), "hipMalloc(V chunk)"))
        return -1;
    double *wao = (double *)s->ao_ws.p, *vt = (double *)s->vtmp.p, *eacc = vt + (size_t)nao * nao;
    const double *coords = (const double *)d_coords, *w = (const double *)d_w;
    const unsigned nb = (unsigned)(((size_t)nao * nao + 255) / 256);
    for (long g0 = 0; g0 < (long)ngrid; g0 += chunk) {
        const long n = std::min<long>(chunk, (long)ngrid - g0);
        double *wgr = gga ? wao + (size_t)n * nao : nullptr;       // (3, n, nao) right behind the values of THIS chunk
        launch_ao(s, tab, n, nao, coords + 3 * g0, wao, wgr);
        if (!xc_sweep(s, n, nao, (const double *)d_dm, wao, wgr, w + g0, vt, false)) return -1;
        hipLaunchKernelGGL(k_accumulate_chunk, dim3(nb), dim3(256), 0, s->stream, (long)nao * nao, g0 == 0 ? 0 : 1, vt,
                           (const double *)s->exc.p, (double *)d_vxc, eacc);
    }
    if (d_exc && !hip_ok(s, hipMemcpyAsync((void *)d_exc, eacc, sizeof(double), hipMemcpyDeviceToDevice, s->stream), "copy Exc"))
        return -1;
    return hip_ok(s, hipGetLastError(), "direct XC sweep launch") ? 0 : -1;
}

int DFT_SetOption(XCSolver *s, const char *key, double value)
{
    if (!s || !key) return -1;
    if (strcmp(key, "profile") && strcmp(key, "spin_wait") && strcmp(key, "strict_sync")) {
        DeviceGuard dg(s);
        drop_graphs(s); // recorded sweeps were launched under the old options
    }
    if (!strcmp(key, "eri_symmetric")) { s->eri_sym = value == 2.0 ? 2 : value != 0.0; return 0; }
    if (!strcmp(key, "graph")) { s->graph = value > 0.0 ? 1 : value < 0.0 ? -1 : 0; return 0; }
    if (!strcmp(key, "quirks")) { s->quirks = value != 0.0; s->fxc[0].ngrid = 0; return 0; }   // the prepared kind-0 table held the old formulas
    if (!strcmp(key, "path")) { s->path = (int)value; return 0; }
    if (!strcmp(key, "profile")) { s->profile = value != 0.0; return 0; }
    if (!strcmp(key, "spin_wait")) { s->spin_wait = value != 0.0; return 0; }
    if (!strcmp(key, "strict_sync")) { s->strict_sync = value != 0.0; return 0; }
    if (!strcmp(key, "fuse_finish")) { s->fuse_finish = value != 0.0; return 0; }
    if (!strcmp(key, "vxc_fringe")) { s->vxc_fringe = value > 0.0 ? 1 : value < 0.0 ? -1 : 0; return 0; }
    if (!strcmp(key, "publish")) { s->publish = value > 0.0 ? 1 : value < 0.0 ? -1 : 0; return 0; }
    if (!strcmp(key, "sweep_order")) { s->sweep_order = (int)value & 3; return 0; }
    if (!strcmp(key, "occ")) { s->occ = value == 1.0 ? 1 : value == 2.0 ? 2 : 0; return 0; }
    if (!strcmp(key, "dm_factor")) { s->dm_factor = value != 0.0; return 0; }
    if (!strcmp(key, "tiny")) { s->tiny = value > 0.0 ? 1 : value < 0.0 ? -1 : 0; return 0; }
    if (!strcmp(key, "ao_pt")) { s->ao_pt = value == 16.0 ? 16 : value == 8.0 ? 8 : 0; return 0; }
    if (!strcmp(key, "ksplit")) { s->ksplit = value > 0 ? (int)value : 0; return 0; }
    if (!strcmp(key, "xcg_spin_fused")) { s->xcg_spin_fused = value != 0.0; return 0; }
    if (!strcmp(key, "meta_fused")) { s->meta_fused = value != 0.0; return 0; }
    if (!strcmp(key, "xcg_meta_fused")) { s->xcg_meta_fused = value != 0.0; return 0; }
    if (!strcmp(key, "xcg_meta_spin_fused")) { s->xcg_meta_spin_fused = value != 0.0; return 0; }
    if (!strcmp(key, "tau_spin_fused")) { s->tau_spin_fused = value != 0.0; return 0; }
    return -1;
}

double DFT_GetOption(XCSolver *s, const char *key)
{
    const double unknown = std::numeric_limits<double>::quiet_NaN();
    if (!s || !key) return unknown;
    if (!strcmp(key, "publish")) return s->publish;
    if (!strcmp(key, "publish_probe")) return s->publish_ok ? 1.0 : 0.0;                        // the creation-time probe's verdict
    if (!strcmp(key, "publish_live")) return s->publish > 0 && s->publish_ok ? 1.0 : 0.0;      // what a default-path call does now
    if (!strcmp(key, "used_publish")) return s->used_publish;                                   // what the last synchronous call did
    if (!strcmp(key, "vxc_fringe")) return s->vxc_fringe;
    if (!strcmp(key, "used_vxc_fringe")) return s->used_vxc_fringe;                            // what the last sweep's Vxc kernel was
    if (!strcmp(key, "fuse_finish")) return s->fuse_finish;
    if (!strcmp(key, "strict_sync")) return s->strict_sync;
    if (!strcmp(key, "spin_wait")) return s->spin_wait;
    if (!strcmp(key, "graph")) return s->graph;
    if (!strcmp(key, "tiny")) return s->tiny;
    if (!strcmp(key, "sweep_order")) return s->sweep_order;
    if (!strcmp(key, "path")) return s->path;
    if (!strcmp(key, "quirks")) return s->quirks;
    if (!strcmp(key, "occ")) return s->occ;
    if (!strcmp(key, "used_occ")) return s->used_occ;                                          // what the last sweep's density step was
    if (!strcmp(key, "dm_factor")) return s->dm_factor;
    if (!strcmp(key, "used_dm_factor")) return s->used_dm_factor;                              // the last synchronous call swept with the factor of dm
    if (!strcmp(key, "xcg_spin_fused")) return s->xcg_spin_fused;
    if (!strcmp(key, "meta_fused")) return s->meta_fused;
    if (!strcmp(key, "xcg_meta_fused")) return s->xcg_meta_fused;
    if (!strcmp(key, "xcg_meta_spin_fused")) return s->xcg_meta_spin_fused;
    if (!strcmp(key, "tau_spin_fused")) return s->tau_spin_fused;
    if (!strcmp(key, "dm_factor_rank")) return s->dm_factor_rank;                              // the rank its attempt found (0: rejected / not attempted)
    return unknown;
}

int DFT_SetStream(XCSolver *s, unsigned long long hip_stream)
{
    if (!s) return -1;
    DeviceGuard dg(s);
    if (s->device_ok) (void)hipStreamSynchronize(s->stream);
    s->stream = (hipStream_t)hip_stream;
    return 0; // recorded sweeps are stream-independent (recorded on the solver's own stream, launched on the current one)
}

const char *DFT_GetLastError(XCSolver *s)
{
    return s ? s->last_error.c_str() : "";
}

int DFT_GetTimings(XCSolver *s, double *ms, const char **names, int max_entries)
{
    if (!s || !s->device_ok) return 0;
    DeviceGuard dg(s);
    (void)hipStreamSynchronize(s->stream);
    int n = 0;
    for (size_t i = 0; i < s->n_timed && n < max_entries; ++i, ++n) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, s->timings[i].t0, s->timings[i].t1) != hipSuccess) t = -1.f;
        if (ms) ms[n] = t;
        if (names) names[n] = s->timings[i].name;
    }
    return n;
}

} // extern "C"
