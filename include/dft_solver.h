/*
 * dft_solver.h -- C-ABI of the MI355X-native XC/Fock engine (libdft.so).
 *
 * Drop-in boundary: the first four entry points are exactly the four
 * `extern "C"` symbols of the reference (src/dft_solver.h:66-88, defined at
 * src/dft_solver.cu:675-719) that its ctypes wrapper binds (dft.py:24-50):
 * same names, argument order, types and error behaviour.  Everything after
 * them is a non-breaking extension (new symbols only).
 *
 * All pointers are raw *device* addresses passed as 64-bit integers, exactly
 * as the reference's caller does (`cupy_array.data.ptr`, dft.py:69-95).  All
 * arrays are fp64, C-contiguous:
 *   dm (nao,nao) | ao (ngrid,nao) | ao_grad (3,ngrid,nao) planar | weights (ngrid)
 *   vxc (nao,nao) overwritten | eri (nao^2,nao^2) | J, K (nao,nao) overwritten.
 * Work is enqueued on the solver's stream (default: the null stream, like the
 * reference); DFT_ComputeXC returns Exc once the call's last kernel -- a one-block
 * finishing kernel that stream order starts after every other kernel of the call
 * has completed -- has published it: on return Vxc is complete for consumers on
 * any stream, as after the reference's blocking copy (dft_solver.cu:575-582).
 * (Option "fuse_finish" = 1 trades that for one launch less: see DFT_SetOption.)
 * Every entry point runs on the device that was current at DFT_CreateSolver.
 * No function throws or aborts; failures print one line to stderr, are
 * retrievable with DFT_GetLastError(), and make DFT_ComputeXC return NaN.
 */
#ifndef QCDFT_AMD_DFT_SOLVER_H
#define QCDFT_AMD_DFT_SOLVER_H

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque handle; replaces the reference's `class XCSolver` hierarchy
 * (src/dft_solver.h:7-63: XCSolver / LDASolver / GGASolver / B3LYPSolver). */
typedef struct XCSolver XCSolver;

/* src/dft_solver.h:67-71 */
enum SolverType { SOLVER_LDA = 0, SOLVER_GGA = 1, SOLVER_B3LYP = 2,
                  SOLVER_MIX = 3 /* extension: a weighted sum of components, DFT_CreateSolverMix only */ };

/* The pointwise components a mix solver can combine (extension), in the order of its weight vector. */
enum XCComponent { XC_SLATER_X = 0, XC_VWN5_C, XC_VWN_RPA_C, XC_PW92_C,
                   XC_PBE_X, XC_PBE_C, XC_B88_X, XC_LYP_C, XC_NCOMP };

/* ---- reference ABI ------------------------------------------------------ */

/* src/dft_solver.h:73, src/dft_solver.cu:677-682.  Unknown type -> NULL. */
XCSolver *DFT_CreateSolver(int type);

/* src/dft_solver.h:75, src/dft_solver.cu:684-686.  NULL is a no-op. */
void DFT_DestroySolver(XCSolver *solver);

/* src/dft_solver.h:77-82, src/dft_solver.cu:688-704 -> {LDA,GGA,B3LYP}Solver::
 * compute_xc (:559-672).  Returns Exc = sum_g w_g rho_g eps_xc(g) and
 * overwrites vxc:  LDA/B3LYP symmetric; GGA the reference's one-sided matrix
 * (the caller averages it, dft.py:212).  d_ao_grad_ptr may be 0 for LDA.
 * NULL solver -> 0.0 (src/dft_solver.cu:695). */
double DFT_ComputeXC(XCSolver *solver, int ngrid, int nao,
                     unsigned long long d_dm_ptr,
                     unsigned long long d_ao_ptr,
                     unsigned long long d_ao_grad_ptr,
                     unsigned long long d_weights_ptr,
                     unsigned long long d_vxc_ptr);

/* src/dft_solver.h:84-87, src/dft_solver.cu:706-718 -> XCSolver::
 * compute_coulomb (:550-555).  J.ravel() = ERI^T . D.ravel() (the cublasDgemv
 * OP_N call on the row-major buffer).  Asynchronous on the solver's stream.
 * NULL solver -> no-op (src/dft_solver.cu:711). */
void DFT_ComputeCoulomb(XCSolver *solver, int nao,
                        unsigned long long d_eri_ptr,
                        unsigned long long d_dm_ptr,
                        unsigned long long d_J_ptr);

/* ---- extensions (not in the reference) ---------------------------------- */

/* ABI version of this library (bumped when an extension changes). */
int DFT_GetVersion(void);

/* A solver for a MIXED functional: eps = sum_k weights[k] eps_k over the XC_NCOMP components above (type SOLVER_MIX;
 * DFT_CreateSolver(SOLVER_MIX) stays NULL, it has no weights).  NULL unless ncomp == XC_NCOMP, every weight is finite
 * and at least one is non-zero; negative weights are allowed.  The weights are fixed for the solver's life (recorded
 * HIP graphs hold them): there is no setter.  Per grid point with rho >= 1e-12 (below: no contribution, as in the
 * three built-in bodies):
 *     e = sum c_k e_k    vrho = sum c_k vrho_k    vsigma = sum c_k vsigma_k
 *     B88 in its closed-shell form, as the B3LYP body takes it: b88(rho/2, sigma/4), vsigma halved
 *     Exc += w rho e     B[g,:] = w vrho phi + 4 w vsigma (grad rho . grad phi)     V = B^T phi
 * i.e. the GGA convention of DFT_ComputeXC whatever the components: factor 4, a ONE-SIDED matrix, no symmetrisation
 * in the library -- the caller takes (V + V^T)/2, as the driver and DFT_ScfTailStep do for every type.  With B3LYP's
 * coefficients that average equals SOLVER_B3LYP's output (which halves vrho, uses factor 2 and adds M + M^T).
 * Option "quirks" keeps its meaning for XC_VWN5_C and XC_PBE_C.  With weights XC_PBE_X..XC_LYP_C all zero the solver
 * is an LDA-class one (one-plane kernels, d_ao_grad_ptr may be 0); otherwise a null ao_grad is the error it is for
 * SOLVER_GGA.  A component with weight 0 is not evaluated.  Every entry that takes an XCSolver* accepts a mix solver. */
XCSolver *DFT_CreateSolverMix(const double *weights, int ncomp);

/* The weights of a mix solver, or the equivalent of a built-in type under the convention above (LDA: slater 1,
 * vwn5 1; GGA: pbe_x 1, pbe_c 1; B3LYP: slater 0.80, b88 0.72, vwn_rpa 0.19, lyp 0.81).  0, or -1 for a null handle
 * or ncomp != XC_NCOMP. */
int DFT_GetMix(XCSolver *solver, double *weights_out, int ncomp);

/* Same as DFT_ComputeXC with a 64-bit grid count (the reference's `int`
 * products overflow once ngrid*nao >= 2^30, src/dft_solver.cu:597,634). */
double DFT_ComputeXC64(XCSolver *solver, long long ngrid, int nao,
                       unsigned long long d_dm_ptr,
                       unsigned long long d_ao_ptr,
                       unsigned long long d_ao_grad_ptr,
                       unsigned long long d_weights_ptr,
                       unsigned long long d_vxc_ptr);

/* DFT_ComputeXC with the OCCUPIED ORBITALS of the density: d_cocc_ptr (nao, nocc) f64 C-order with
 * dm = cocc . cocc^T (occupation folded in: sqrt(2) C_occ for the closed-shell dm of dft.py:181-182; the
 * same contract as DFT_ComputeJKFactorized).  Same results as DFT_ComputeXC(dm) -- same Exc, same Vxc
 * conventions per solver type -- but the density step runs as Y = AO . cocc, rho = rowsum(Y^2),
 * X = Y . cocc^T, grad rho = 2 rowsum(X * dAO): 4 nao nocc flops per grid point on the matrix cores instead
 * of the 2 nao^2 of the reference's contraction with the full matrix (dft_solver.cu:294-307, 346-380).
 * d_dm_ptr may be 0; where the occupied form does not do fewer matrix instructions (nocc close to nao/2:
 * minimal basis sets) the library takes the dm path, with the caller's dm if given, else with cocc . cocc^T
 * formed on the device.  A dm that is NOT cocc . cocc^T is the caller's error (the result then follows cocc
 * or dm depending on the path taken).  Returns Exc like DFT_ComputeXC. */
double DFT_ComputeXCOcc(XCSolver *solver, long long ngrid, int nao, int nocc,
                        unsigned long long d_cocc_ptr,
                        unsigned long long d_dm_ptr,
                        unsigned long long d_ao_ptr,
                        unsigned long long d_ao_grad_ptr,
                        unsigned long long d_weights_ptr,
                        unsigned long long d_vxc_ptr);

/* Asynchronous form of DFT_ComputeXCOcc (see DFT_ComputeXCAsync). */
int DFT_ComputeXCOccAsync(XCSolver *solver, long long ngrid, int nao, int nocc,
                          unsigned long long d_cocc_ptr,
                          unsigned long long d_dm_ptr,
                          unsigned long long d_ao_ptr,
                          unsigned long long d_ao_grad_ptr,
                          unsigned long long d_weights_ptr,
                          unsigned long long d_vxc_ptr,
                          unsigned long long d_exc_ptr);

/* Asynchronous form: Exc is written to the device double at d_exc_ptr; no
 * host synchronisation.  Returns 0 on success. */
int DFT_ComputeXCAsync(XCSolver *solver, long long ngrid, int nao,
                       unsigned long long d_dm_ptr,
                       unsigned long long d_ao_ptr,
                       unsigned long long d_ao_grad_ptr,
                       unsigned long long d_weights_ptr,
                       unsigned long long d_vxc_ptr,
                       unsigned long long d_exc_ptr);

/* Exact exchange on the dense ERI, replaces the driver's
 * cp.einsum('ijkl,jl->ik', eri4d, dm) (dft.py:218).  Asynchronous. */
void DFT_ComputeExchange(XCSolver *solver, int nao,
                         unsigned long long d_eri_ptr,
                         unsigned long long d_dm_ptr,
                         unsigned long long d_K_ptr);

/* J and K from ONE pass over the dense ERI (dft.py:203 + dft.py:218).
 * Either output pointer may be 0. */
void DFT_ComputeJK(XCSolver *solver, int nao,
                   unsigned long long d_eri_ptr,
                   unsigned long long d_dm_ptr,
                   unsigned long long d_J_ptr,
                   unsigned long long d_K_ptr);

/* The same contractions restricted to ERI rows (i, j) with i_lo <= i < i_hi: d_eri_rows points at row
 * (i_lo, 0) of the (nao^2, nao^2) matrix, i.e. at a rank's resident ROW BLOCK when the dense ERI is
 * sharded over GPUs (the reference is single-GPU, dft_solver.cu:550-555 / dft.py:218 are the
 * whole-matrix forms).  J receives this block's partial sum over rows for EVERY column (the reference's
 * OP_N dgemv is a sum over rows), K receives rows [i_lo, i_hi) and zeros elsewhere: summing the outputs of
 * all blocks (one all-reduce) gives the whole-matrix J and K.  Either output may be 0.  Asynchronous;
 * returns 0 or -1 (DFT_GetLastError). */
int DFT_ComputeJKRows(XCSolver *solver, int nao, int i_lo, int i_hi,
                      unsigned long long d_eri_rows,
                      unsigned long long d_dm,
                      unsigned long long d_J,
                      unsigned long long d_K);

/* J and K from a factorised ERI, (ij|kl) ~= sum_P L[P][i][j] L[P][k][l] (pivoted
 * Cholesky vectors, d_chol_ptr: (naux, nao, nao) f64 C-order, every L[P] symmetric).
 * Same matrices as DFT_ComputeCoulomb (dft_solver.cu:550-555, dft.py:203) and the
 * exchange einsum (dft.py:218) to within the factorisation threshold, for basis sizes
 * whose dense ERI (8 nao^4 bytes) does not fit in HBM; K runs as fp64 MFMA GEMMs.
 * d_cocc_ptr: (nao, nocc) f64 C-order with dm = cocc . cocc^T (occupation folded in,
 * i.e. sqrt(2) C_occ for the closed-shell dm of dft.py:181-182).  d_J_ptr or d_K_ptr
 * may be 0; J needs d_dm_ptr, K needs d_cocc_ptr.  When BOTH are requested the contraction
 * L_P : dm that J needs rides in the K build (taken from the half-transformed vectors and
 * cocc) as long as dm IS cocc . cocc^T -- checked on the device in every call; for any other
 * dm (damped, mixed, fractional occupations) J contracts dm itself in a pass of its own.
 * Asynchronous; returns 0 or -1 (DFT_GetLastError). */
int DFT_ComputeJKFactorized(XCSolver *solver, int nao, int naux, int nocc,
                            unsigned long long d_chol_ptr,
                            unsigned long long d_dm_ptr,
                            unsigned long long d_cocc_ptr,
                            unsigned long long d_J_ptr,
                            unsigned long long d_K_ptr);

/* Response J and K from the same vectors for nvec trial densities that share their left factor,
 *     D_k = A B_k^T + B_k A^T,   d_a_ptr: A (nao, nocc),  d_b_ptr: B (nvec, nao, nocc), f64 C-order
 * (what an excitation or CPKS solver has: A the occupied orbitals, B_k a trial vector in the AO basis):
 *     d_J_ptr (nvec, nao, nao) or 0:  J_k = sum_P (L_P : D_k) L_P
 *     d_M_ptr (nvec, nao, nao) or 0:  M_k = sum_P (L_P A)(L_P B_k)^T, NOT symmetrised:
 *         K[D]_mn = sum_ls (ml|ns) D_ls  gives  K[A B_k^T +- B_k A^T] = M_k +- M_k^T,
 *     so the exchange response of an antisymmetric density, which no combination of
 *     DFT_ComputeJKFactorized calls expresses, comes from the same M.
 * Cost: A is half-transformed once per call; L_P : D_k is taken from that half transform, not from L;
 * J of up to 8 trials takes ONE pass over L (larger nvec: groups of 8); M takes one half transform of
 * B_k and one fp64-MFMA product per trial.  A trial's J and M are bitwise the same whether it is sent
 * alone or in a batch.  Both outputs 0: returns 0, nothing is launched.  Asynchronous; returns 0, or -1
 * for bad sizes (nao, naux, nocc, nvec <= 0) or a null input (DFT_GetLastError).  DFT_GetVersion is
 * unchanged: look the symbol up. */
int DFT_ComputeJKFactorizedResponse(XCSolver *solver, int nao, int naux, int nocc, int nvec,
                                    unsigned long long d_chol_ptr,
                                    unsigned long long d_a_ptr,
                                    unsigned long long d_b_ptr,
                                    unsigned long long d_J_ptr,
                                    unsigned long long d_M_ptr);

/* AO values (and Cartesian gradients) on the grid: replaces PySCF's
 * dft.numint.eval_ao(mol, coords, deriv=0/1) at grid.py:30,38.
 * Shell table (host pointers, copied to the device on first use / change):
 *   nshell shells; shell s: centre (x,y,z) bohr in shl_xyz[3s..], angular
 *   momentum shl_l[s] (0..3), shl_nprim[s] primitives starting at
 *   shl_off[s] in prim_exp / prim_coef (coefficients already include the
 *   primitive and contraction normalisation), first AO column shl_ao[s].
 * coords (ngrid,3) device; ao (ngrid,nao) device out; ao_grad (3,ngrid,nao)
 * device out or 0.  Returns 0 on success. */
int DFT_EvalAO(XCSolver *solver, long long ngrid, int nao, int nshell,
               const double *shl_xyz, const int *shl_l, const int *shl_nprim,
               const int *shl_off, const int *shl_ao,
               const double *prim_exp, const double *prim_coef, int nprim_total,
               unsigned long long d_coords_ptr,
               unsigned long long d_ao_ptr,
               unsigned long long d_ao_grad_ptr);

/* The whole AO -> rho -> XC -> Vxc sweep without resident AO planes ("fused mode"): what
 * grid.py:30,38 + dft.py:155,172 + DFT_ComputeXC do together, chunk by chunk -- the AO values and gradients of
 * `chunk_points` grid points (0 = automatic: ~96 MB of planes, an Infinity-Cache-sized working set) are evaluated into
 * a workspace of the solver, swept, and overwritten by the next chunk; Vxc and Exc add up over the chunks (the
 * sweep is linear in the grid points).  Memory: chunk_points*nao*(1 or 4) doubles instead of ngrid*nao*(1 or 4)
 * (BASELINE config 5: 53 GB resident); cost: the AO evaluation is repeated in every call.  Shell table as for
 * DFT_EvalAO; coords (ngrid,3), weights (ngrid), dm (nao,nao) device in; vxc (nao,nao) and exc (1 double, may be 0)
 * device out, valid after the work queued on the solver's stream completes (as DFT_ComputeXCAsync).  0 on success. */
int DFT_ComputeXCDirect(XCSolver *solver, long long ngrid, int nao, int nshell,
                        const double *shl_xyz, const int *shl_l, const int *shl_nprim,
                        const int *shl_off, const int *shl_ao,
                        const double *prim_exp, const double *prim_coef, int nprim_total,
                        unsigned long long d_coords_ptr,
                        unsigned long long d_weights_ptr,
                        unsigned long long d_dm_ptr,
                        unsigned long long d_vxc_ptr,
                        unsigned long long d_exc_ptr,
                        long long chunk_points);

/* dm = L L^T on the device, for a caller that holds the density matrix and nothing else (what the reference's loop
 * passes, dft.py:200; its dm = 2 C_occ C_occ^T has the rank of the occupied space): pivoted Cholesky in one workgroup
 * (csrc/dm_factor.hip), then an acceptance check of |dm - L L^T| over the whole matrix with the bound the factorised J/K
 * build uses (1e-11 relative to |L| |L|^T + |dm|, plus 1e-14).  L (nao, rank), C order, is the `cocc` of DFT_ComputeXCOcc
 * and DFT_ComputeJKFactorized.  dm (nao, nao) device in; d_cocc_out: nao * max_rank doubles, device out.  max_rank <= 0
 * means nao / 2 (values above nao are cut to nao), tol <= 0 means 1e-13: the factorisation stops when the largest
 * residual diagonal entry is <= tol * max_i dm_ii.  Synchronous on the solver's stream and device.  Returns
 *   the rank (>= 1): L is in the first nao * rank doubles of d_cocc_out;
 *   0: dm is not such a product with rank <= max_rank (d_cocc_out holds nothing the caller may rely on);
 *   -1: an error (DFT_GetLastError); nothing aborts.
 * info4, if not NULL, receives {steps taken, last residual maximum / scale, reason, scale = max_i dm_ii} with reason
 * 0 = accepted, 1 = max_rank exceeded, 2 = a negative residual or a non-positive (or non-finite) diagonal, 3 = the
 * acceptance check failed (a non-symmetric dm ends here: the factorisation reads pivot rows only; so does one with a
 * NaN or an infinity in it), 4 = nao outside 2..8192.  Added without a change of DFT_GetVersion (it stays 5): a caller
 * that may meet an older library looks the symbol up. */
int DFT_FactorDensity(XCSolver *solver, int nao, unsigned long long d_dm_ptr, int max_rank, double tol,
                      unsigned long long d_cocc_out_ptr, double *info4);

/* Linear response of Vxc: V1 = d/dt DFT_ComputeXC(dm0 + t dm1).vxc at t = 0, element for element the derivative of what
 * DFT_ComputeXC writes for the solver's type and options (one-sided for SOLVER_GGA and SOLVER_MIX, M + M^T with the halved
 * vrho for SOLVER_B3LYP, symmetric for SOLVER_LDA; the caller symmetrises as it does for Vxc).  With option "quirks" = 1
 * that is the derivative of the SHIPPED vrho / vsigma formulas (forward-mode differentiation of the functional bodies),
 * the only definition consistent with DFT_ComputeXC there.  Points with rho below the cut-off contribute nothing; every
 * clamp and cut-off of the bodies takes the branch of the value.
 *
 * DFT_FxcPrepare runs the ground-state density step of a sweep (through d_cocc (nao, nocc), dm0 = cocc cocc^T, under
 * the rule of DFT_ComputeXCOcc when d_cocc is not 0; d_dm0 may then be 0) and keeps the derivative table of the
 * functional and grad rho0 in the solver.  DFT_FxcApply takes any matrix dm1 (its symmetric part counts), the same planes,
 * and leaves V1 in d_v1 (nao, nao): density kernels on dm1, one arithmetic kernel, then the contraction and reduce
 * kernels of the sweep with the sweep's choices ("path", "vxc_fringe", nao, plane size).  No energy, no host wait:
 * asynchronous on the solver's stream.  Apply may be called any number of times after one Prepare; DFT_ComputeXC* calls
 * in between are allowed and change nothing.  Both return 0, or -1 with DFT_GetLastError (nothing aborts): Apply before
 * Prepare, ngrid or nao differing from Prepare's, a null ao_grad on a gradient solver.  DFT_SetOption("quirks") after
 * Prepare invalidates the table.  Added without a change of DFT_GetVersion: look the symbols up. */
int DFT_FxcPrepare(XCSolver *solver, long long ngrid, int nao, int nocc, unsigned long long d_cocc_ptr,
                   unsigned long long d_dm0_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                   unsigned long long d_weights_ptr);
int DFT_FxcApply(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm1_ptr, unsigned long long d_ao_ptr,
                 unsigned long long d_ao_grad_ptr, unsigned long long d_v1_ptr);

/* The same two halves for the response tables of the SPIN-RESOLVED energy bodies (csrc/xc_spin_functionals.hpp), at the
 * closed-shell ground state dm0.  kind 1, triplet: with dm_alpha, dm_beta = dm0/2 +- t dm1/2, V1 is d/dt of the
 * alpha-spin XC potential matrix at t = 0 -- (V1 + V1^T)/2 is that derivative of the symmetric matrix -- in the
 * conventions of DFT_FxcApply for the solver's type (one-sided for SOLVER_GGA and SOLVER_MIX, M + M^T with the halved
 * table for SOLVER_B3LYP, symmetric for SOLVER_LDA).  kind 2, singlet: the same bodies along dm_alpha = dm_beta =
 * (dm0 + t dm1)/2, which is DFT_FxcApply's V1 at "quirks" = 0 to rounding.  The tables are second derivatives of the
 * ENERGY (forward mode of second order through the energy statements): they do not depend on option "quirks", and
 * DFT_SetOption("quirks") does not invalidate them.  At "quirks" = 1 the ground state solves the shipped potentials of
 * vwn5_c and pbe_c, which are not the derivatives of their energies; a caller that needs the response of the equations
 * it solved sets "quirks" = 0 for those components.
 *
 * DFT_FxcPrepareSpin runs the density step of DFT_FxcPrepare (same arguments, same rule for d_cocc) and fills the slot
 * of `kind`: its own table and its own grad rho0, so the two Prepare entries and the Apply entries of every kind
 * interleave freely, at the same or at different dm0, and a DFT_FxcPrepare table is never disturbed.
 * DFT_FxcApplyKind is DFT_FxcApply with the table chosen: kind 0 the DFT_FxcPrepare table, 1 / 2 the slots above; the same
 * host function, the same kernels ("fxc_coef" and the sweep's contraction and reduce).  Both return 0, or -1 with
 * DFT_GetLastError (nothing aborts): an unknown kind, Apply before the Prepare of that kind, ngrid or nao differing from
 * that Prepare's, a null ao_grad on a gradient solver.  Added without a change of DFT_GetVersion (it stays 5): look the
 * symbols up. */
int DFT_FxcPrepareSpin(XCSolver *solver, long long ngrid, int nao, int nocc, unsigned long long d_cocc_ptr,
                       unsigned long long d_dm0_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                       unsigned long long d_weights_ptr, int kind);
int DFT_FxcApplyKind(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm1_ptr, unsigned long long d_ao_ptr,
                     unsigned long long d_ao_grad_ptr, unsigned long long d_v1_ptr, int kind);

/* Open-shell (spin-resolved) sweep: Exc[dm_a, dm_b] into *exc and the XC potential matrices of the two spins,
 *     V_s = d Exc / d dm_s,   s = alpha, beta,
 * into d_vxc_a / d_vxc_b (nao, nao), in the convention DFT_ComputeXC writes Vxc in for the solver's type (one-sided for
 * SOLVER_GGA and SOLVER_MIX -- (V_s + V_s^T)/2 is the symmetric matrix --, M + M^T for SOLVER_B3LYP, symmetric for
 * SOLVER_LDA).  dm_a / dm_b (nao, nao): the spin density matrices (their symmetric parts count); the other arguments
 * as DFT_ComputeXC64.  At dm_a = dm_b = dm/2 and "quirks" = 0 the call gives DFT_ComputeXC(dm)'s Exc and Vxc, twice, to
 * rounding.  The potentials are first derivatives of the spin-resolved ENERGY bodies (csrc/xc_spin_functionals.hpp,
 * forward mode; nothing is differentiated by hand): at "quirks" = 1 a functional with vwn5_c or pbe_c is refused, whose
 * shipped potentials are not those derivatives.  A point where one spin's density is below the cut-off (1e-12) is
 * evaluated as fully polarised: that spin contributes nothing and receives no potential there, the other one gets the
 * zeta = +-1 limit.
 * Order of work on the solver's stream: the density kernels of the sweep on dm_a, then on dm_b, one pointwise kernel
 * ("xc_points_spin"), the sweep's contraction and reduce for alpha, then for beta, with the sweep's choices ("path",
 * "vxc_fringe", nao, plane size) -- never the one-kernel plan for small bases, never a recorded graph, never the
 * occupied-orbital density step.  Synchronous: returns after Exc has been copied to *exc.  Prepared DFT_Fxc* tables and
 * later DFT_ComputeXC* calls are not disturbed.  Returns 0, or -1 with DFT_GetLastError (nothing aborts): a null
 * pointer, bad sizes, a null ao_grad on a gradient solver, the "quirks" case above.  Added without a change of
 * DFT_GetVersion (it stays 5): look the symbol up.
 *
 * DFT_ComputeXCSpin, DFT_ComputeXCMeta and DFT_ComputeXCMetaSpin are one synchronous sweep over the spins of the call
 * (xc_sweep_sync, csrc/dft_api.hip).  Where a call has more than one fault, all three refuse in this order: the solver's
 * kind (a meta entry on a solver without meta weights; DFT_ComputeXCSpin on one with a non-zero meta weight), a null
 * pointer ("... needs ..."; ao_grad counts here for DFT_ComputeXCMetaSpin only), no usable device, bad sizes, a null
 * ao_grad on a gradient solver ("ao_grad pointer is null"), then the "quirks" case.  Nothing has touched the device by
 * then.  The three entries, DFT_ComputeTau / DFT_ComputeTauSpin and the open-shell response pair (DFT_FxcPrepareSpinPol /
 * DFT_FxcApplySpinPol) work in one set of buffers of the solver, in stream order, each call writing whole what it reads:
 * no result of one depends on what another left there, and no recorded graph or prepared table holds any of them.
 *
 * The eight gradient-side entries further down -- DFT_ComputeXCGradient / DFT_ComputeXCGradientSpin / DFT_ComputeXCGradientMeta /
 * DFT_ComputeXCGradientMetaSpin and DFT_ComputeXCEnergyDensity / DFT_ComputeXCEnergyDensitySpin / DFT_ComputeXCEnergyDensityMeta /
 * DFT_ComputeXCEnergyDensityMetaSpin -- are likewise one gradient path
 * and one energy-density path over (spins, meta) with one density stage (xc_gradient, xc_energy_density, xcg_density,
 * csrc/dft_api.hip).  Where a call has more than one fault, all eight refuse in this order: the solver's kind (a meta entry on a
 * solver without meta weights; any other on one with a non-zero meta weight), a null pointer ("... needs ..."; ao_grad and
 * ao_hess count here for the meta entries only), bad sizes, a null ao_grad on a gradient solver ("ao_grad pointer is null"), for
 * the gradients a null ao_hess on a gradient solver ("ao_hess pointer is null") and a null ao_grad on any other ("... needs
 * ao_grad"), the "quirks" case (every entry but the two closed-shell non-meta ones), for the gradients an LDS request above
 * 160 KB, and last no usable device: a caller without a device still learns every fault of its arguments.  Nothing has touched
 * the device by then.  The eight work in one set of buffers of the solver of their own -- the planes
 * and the padded matrix of each spin, tau and its coefficient plane, the slabs of the contraction -- in stream order: an entry
 * reserves what it uses at the size of its call, every call writes whole what it reads, so no result of one depends on what
 * another left there (each is bitwise what a fresh solver gives), and no recorded graph and no prepared table holds any of them. */
int DFT_ComputeXCSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr,
                      unsigned long long d_dm_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                      unsigned long long d_weights_ptr, unsigned long long d_vxc_a_ptr, unsigned long long d_vxc_b_ptr,
                      double *exc);

/* Meta-GGA functionals.  Two further components read the kinetic-energy density
 *     tau(g) = 1/2 sum_k sum_mu,nu D[mu, nu] (d_k phi_mu)(g) (d_k phi_nu)(g):
 * TPSS exchange and TPSS correlation (csrc/xc_meta_functionals.hpp: energies per volume of the spin variables, first
 * derivatives by forward mode, written down as recalled -- the numerical rules are stated there). */
enum XCMetaComponent { XC_TPSS_X = 0, XC_TPSS_C, XC_NMETA };

/* A solver for eps = sum_k weights[k] eps_k + sum_k meta_weights[k] eps_meta_k (type SOLVER_MIX with meta weights; it
 * always takes the four-plane form: ao_grad is required).  NULL unless ncomp == XC_NCOMP, nmeta == XC_NMETA, every
 * weight is finite and at least one is non-zero.  With a non-zero meta weight the solver serves DFT_ComputeTau,
 * DFT_ComputeXCMeta and their open-shell counterparts DFT_ComputeTauSpin / DFT_ComputeXCMetaSpin only: every other XC entry refuses it (-1 / NaN and a sentence in DFT_GetLastError), so that tau
 * cannot be dropped silently.  Added without a change of DFT_GetVersion (it stays 5): look the symbols up. */
XCSolver *DFT_CreateSolverMeta(const double *weights, int ncomp, const double *meta_weights, int nmeta);

/* The meta weights of a solver (zeros for one made by DFT_CreateSolver / DFT_CreateSolverMix).  0, or -1 for a null
 * argument or nmeta != XC_NMETA. */
int DFT_GetMeta(XCSolver *solver, double *meta_weights_out, int nmeta);

/* d_tau (ngrid) receives tau of d_dm (nao, nao; its symmetric part) from the three gradient planes d_ao_grad
 * (3, ngrid, nao): "tau" (k_tau, csrc/xc_meta.hip) on the matrix pipe, no atomics, bitwise reproducible.  Asynchronous
 * on the solver's stream.  Any solver.  0, or -1 with DFT_GetLastError. */
int DFT_ComputeTau(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr, unsigned long long d_ao_grad_ptr,
                   unsigned long long d_tau_ptr);

/* Exc and Vxc of a meta solver.  d_vxc (nao, nao) receives V in the mix solver's one-sided convention plus the whole
 * (symmetric) tau term: (V + V^T)/2 is dExc/dD, tr(sym(V) X) = d/dt Exc(D + t X) for symmetric X.  The potentials are
 * first derivatives of the spin-resolved ENERGY bodies at zero polarisation: "quirks" = 1 with a vwn5_c or pbe_c weight
 * is refused (DFT_ComputeXCSpin's reason); TPSS itself carries neither.  A point below the density cut-off contributes
 * exact zeros.
 * Order of work on the solver's stream: the sweep's density kernels on dm, "tau", "xc_points_meta", the sweep's
 * contraction and reduce of c0..c3, then T = sum_k (d_k AO)^T diag(ct) (d_k AO) added to V -- three runs of the sweep's
 * contraction with the plane of d_k AO in the AO slot (option "meta_fused" = 0, the default: the faster form as measured,
 * profiles/meta_time.txt) or one kernel over the three planes ("vxc_tau", "meta_fused" = 1, tested against the plain form).  With both meta weights zero the tau steps are left
 * out.  Never the one-kernel plan for small bases, never a recorded graph, never the occupied-orbital density step.
 * Synchronous: returns after Exc has been copied to *exc.  Prepared DFT_Fxc* tables and later DFT_ComputeXC* calls are
 * not disturbed (the buffers: see DFT_ComputeXCSpin).  Returns 0, or -1 with DFT_GetLastError: a solver not made by
 * DFT_CreateSolverMeta, a null pointer (ao_grad included), bad sizes, the "quirks" case above. */
int DFT_ComputeXCMeta(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr, unsigned long long d_ao_ptr,
                      unsigned long long d_weights_ptr, unsigned long long d_ao_grad_ptr, unsigned long long d_vxc_ptr,
                      double *exc);

/* Meta-GGA functionals, open shell.  d_tau_a, d_tau_b (ngrid each) receive tau of d_dm_a, d_dm_b (their symmetric parts)
 * from the three gradient planes.  Option "tau_spin_fused" = 1 (the default: the faster form as measured,
 * profiles/meta_spin_time.txt): "tau_spin" (k_tau_spin, csrc/xc_meta_spin.hip), one staging of the gradient rows for both
 * spins; 0: k_tau once per spin ("tau x2"), what the tests hold the two-spin kernel to.  Either way no atomics, bitwise reproducible, and per spin the operations of
 * DFT_ComputeTau.  Asynchronous on the solver's stream.  Any solver.  0, or -1 with DFT_GetLastError (bad sizes, a null
 * pointer).  Added without a change of DFT_GetVersion: look the symbols up. */
int DFT_ComputeTauSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr, unsigned long long d_dm_b_ptr,
                       unsigned long long d_ao_grad_ptr, unsigned long long d_tau_a_ptr, unsigned long long d_tau_b_ptr);

/* Exc and the two spin potentials of a meta solver at the spin density matrices d_dm_a, d_dm_b.  d_vxc_s (nao, nao)
 * receives V_s in the mix solver's one-sided convention (DFT_ComputeXCSpin's, scale 1) plus the whole (symmetric) tau term
 * of spin s: (V_s + V_s^T)/2 is dExc/dD_s.  At dm_a = dm_b = dm/2 both are DFT_ComputeXCMeta's V.  A spin channel whose
 * density is below the cut-off at a point is absent there (exact zeros in its coefficients, the zeta = +-1 rules of
 * csrc/xc_meta_functionals.hpp for the other): a spin without electrons gets V_s = 0 exactly.
 * Order of work on the solver's stream: the sweep's density kernels per spin, tau per spin (DFT_ComputeTauSpin's two
 * forms), "xc_points_meta_spin" (xc::meta_spin_point: seven first derivatives by forward mode), the sweep's contraction
 * and reduce of c0..c3 per spin, then the tau term per spin in the form "meta_fused" chooses.  With both meta weights
 * zero tau is cleared instead of computed and the tau terms are left out.  Never the one-kernel plan for small bases,
 * never a recorded graph.  Synchronous.  Prepared DFT_Fxc* tables and later DFT_ComputeXC, DFT_ComputeXCSpin and
 * DFT_ComputeXCMeta calls are not disturbed (the buffers: see DFT_ComputeXCSpin).  Returns 0, or -1 with DFT_GetLastError and no kernel
 * launched: a solver not made by DFT_CreateSolverMeta, a null pointer (ao_grad included), bad sizes, "quirks" = 1 with a
 * vwn5_c or pbe_c weight. */
int DFT_ComputeXCMetaSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr, unsigned long long d_dm_b_ptr,
                          unsigned long long d_ao_ptr, unsigned long long d_weights_ptr, unsigned long long d_ao_grad_ptr,
                          unsigned long long d_vxc_a_ptr, unsigned long long d_vxc_b_ptr, double *exc);

/* Linear response of DFT_ComputeXCSpin, in two halves like DFT_FxcPrepare / DFT_FxcApply: V1_s (nao, nao), s = alpha,
 * beta, is, element for element, d/dt of what DFT_ComputeXCSpin(dm0_a + t dm1_a, dm0_b + t dm1_b) writes into vxc_s at
 * t = 0, in that call's conventions (one-sided for SOLVER_GGA and SOLVER_MIX, M + M^T with the halved table for
 * SOLVER_B3LYP, symmetric for SOLVER_LDA).  Only the symmetric parts of dm1_a / dm1_b count.  At dm0_a = dm0_b = dm0/2,
 * dm1_a = dm1_b = dm1/2 gives V1_a = V1_b = DFT_FxcApplyKind(kind 2)'s V1, and dm1_a = -dm1_b = dm1/2 gives V1_a = -V1_b =
 * kind 1's.
 * DFT_FxcPrepareSpinPol, on the solver's stream: the density kernels of the sweep on dm0_a, then on dm0_b, exactly as
 * DFT_ComputeXCSpin runs them, and the pointwise table ("fxc_table_pol", csrc/xc_response_pol.hip): with x = (rho_a,
 * rho_b, sigma_aa, sigma_ab, sigma_bb) the weighted second derivatives H_ij of the spin-resolved ENERGY bodies and the
 * first derivatives by the three sigmas, forward mode of second order, nothing differentiated by hand; independent of
 * "quirks", but at "quirks" = 1 a functional with vwn5_c or pbe_c is refused for DFT_ComputeXCSpin's reason, in its
 * sentence.  3 planes for an LDA-class functional; 28 otherwise: the 15 of the symmetric H, 3 first derivatives, and
 * the 10 pairs in the other order, which differ from the first 10 only at a sigma cut-off of PBE exchange or
 * correlation (the potential's variable keeps its derivative there, the perturbation sees a constant).  A point where
 * one spin's density is below the cut-off (1e-12): that spin neither responds nor is responded to, its rows and columns
 * are exactly 0; nothing is NaN or Inf.  The table and grad rho0_a, grad rho0_b stay in a slot of their own: the
 * DFT_FxcPrepare table and the kind-1 and kind-2 slots are not disturbed, and neither they nor DFT_ComputeXC* /
 * DFT_ComputeXCSpin calls in between disturb it.
 * DFT_FxcApplySpinPol, asynchronous on the solver's stream, no host wait: the density kernels on dm1_a, then on dm1_b,
 * one arithmetic kernel ("fxc_coef_pol") that couples the two spins, the sweep's contraction and reduce for alpha,
 * then for beta, with the sweep's choices ("path", "vxc_fringe", nao, plane size) -- like DFT_ComputeXCSpin never the
 * one-kernel plan, a recorded graph or the occupied-orbital density step.  Any number of Applies after one Prepare.
 * Both return 0, or -1 with DFT_GetLastError (nothing aborts): a null pointer, bad sizes, a null ao_grad on a gradient
 * solver, Apply before Prepare or with another ngrid / nao, the "quirks" case.  Added without a change of DFT_GetVersion
 * (it stays 5): look the symbols up. */
int DFT_FxcPrepareSpinPol(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm0_a_ptr,
                          unsigned long long d_dm0_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                          unsigned long long d_weights_ptr);
int DFT_FxcApplySpinPol(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm1_a_ptr,
                        unsigned long long d_dm1_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                        unsigned long long d_v1_a_ptr, unsigned long long d_v1_b_ptr);

/* For the tests: copies the table DFT_FxcPrepareSpinPol left (planes as listed at the top of csrc/xc_response_pol.hip, SoA,
 * ngrid doubles each) to d_out on the solver's stream.  Returns the number of planes (3 or 28), or -1 with
 * DFT_GetLastError: nothing prepared, or max_doubles below planes * ngrid. */
int DFT_FxcSpinPolTable(XCSolver *solver, unsigned long long d_out_ptr, long long max_doubles);

/* XC part of the analytic nuclear gradient, at fixed quadrature points and weights (csrc/xc_grad.hip).
 * DFT_EvalAOHess: the six second-derivative planes d_hess (6, ngrid, nao), row-major fp64, in the order xx, xy, xz, yy,
 * yz, zz, of the AOs DFT_EvalAO evaluates: the same shell table (host arrays), real solid harmonics, column order and
 * primitive cut-off (exp(-46)), s-f.  A kernel of its own ("eval_ao_hess"); asynchronous on the solver's stream.
 * DFT_ComputeXCGradient: d_out (nao, 3) receives G[mu, x] = d/dt of the Exc DFT_ComputeXC returns when, in column mu
 * only, ao[:, mu] is replaced by ao[:, mu] - t ao_grad[x][:, mu] and ao_grad[k][:, mu] by ao_grad[k][:, mu] -
 * t ao_hess[xk][:, mu], dm (symmetric) and the weights fixed: the derivative of Exc by the centre of function mu.  The
 * XC term of dE/dR_A is the sum of G[mu, :] over the functions on atom A (taken by the caller).  With "quirks" = 1 and
 * vwn5_c or pbe_c in the functional the shipped potentials are not the derivatives of the energy, and G is built from
 * the shipped ones.  Linear in the grid points: a caller may sum G over slices of the grid.
 * On the solver's stream, no host wait: the density kernels and the pointwise kernel of the sweep with the sweep's
 * choices ("path", nao, plane size), into the gradient entries' set of buffers (see DFT_ComputeXCSpin), then "xc_grad": per tile of 16 grid rows X = AO D and
 * Z = Q D (Q = 2 c0 AO + sum_k c_k ao_grad[k]) on the fp64 matrix pipe, contracted with ao_grad and ao_hess into one
 * (nao, 3) slab per workgroup, and a fixed-order slab sum, so a call is bitwise reproducible.  Never the one-kernel
 * plan, never a recorded graph; prepared DFT_Fxc* tables and later DFT_ComputeXC results are left bit for bit as they
 * were.  d_ao_hess may be 0 for an LDA-class solver (it is not read); d_ao_grad is needed by every solver, since the
 * displaced density is made of it.  nao is limited by the (nao, 3) accumulator and the 16-row AO and Q tiles a
 * workgroup keeps in LDS (tiles of at most 512 columns; wider bases are staged in chunks).
 * Both return 0, or -1 with DFT_GetLastError (nothing aborts): a null pointer, bad sizes, a null ao_grad, a null
 * ao_hess on a gradient solver.  Added without a change of DFT_GetVersion (it stays 5): look the symbols up. */
int DFT_EvalAOHess(XCSolver *solver, long long ngrid, int nao, int nshell,
                   const double *shl_xyz, const int *shl_l, const int *shl_nprim, const int *shl_off, const int *shl_ao,
                   const double *prim_exp, const double *prim_coef, int nprim_total,
                   unsigned long long d_coords_ptr, unsigned long long d_hess_ptr);
int DFT_ComputeXCGradient(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr,
                          unsigned long long d_ao_ptr, unsigned long long d_weights_ptr, unsigned long long d_ao_grad_ptr,
                          unsigned long long d_ao_hess_ptr, unsigned long long d_out_ptr);
/* The same for an open-shell state: d_out (nao, 3) receives G[mu, x] = d/dt of the Exc DFT_ComputeXCSpin(dm_a, dm_b)
 * returns under DFT_ComputeXCGradient's column replacement, both matrices (symmetric) and the weights fixed.  With the
 * per-spin coefficients c_s0..c_s3 of the spin-resolved pointwise kernel (closed-shell conventions)
 *   G[mu, x] = -fac sum_s sum_g [ d_x phi_mu Z_s + (sum_k c_sk d_xk phi_mu) X_s ][g, mu],  X_s = AO D_s,  Z_s = Q_s D_s,
 * Q_s = 2 c_s0 AO + sum_k c_sk ao_grad[k], fac = 1 (one-sided types) or 2 (B3LYP): the closed-shell formula once per spin.
 * On the solver's stream, no host wait: the density kernels on dm_a and on dm_b and the spin-resolved pointwise kernel
 * exactly as DFT_ComputeXCSpin runs them, into the gradient entries' set of buffers, then "xc_grad_spin": k_xc_grad on both spins stages the AO
 * rows of a tile once beside the Q rows of both spins, forms X_a, X_b, Z_a, Z_b of a column tile together and reads each
 * gradient and Hessian plane element once, for d_x phi (Z_a + Z_b) + sum_k d_xk phi (c_ak X_a + c_bk X_b), into one
 * (nao, 3) slab per workgroup; a fixed-order slab sum finishes, so a call is bitwise reproducible.  Option
 * "xcg_spin_fused" = 0 runs k_xc_grad once per spin into two slab sets and one sum over both instead (the same numbers to
 * rounding; 1.6 x / 1.2 x the time at 143 556 x 114 / 60 000 x 494).  Three 16-row tiles: K chunks of at most 320 columns.
 * Linear in the grid points: a caller may sum G over slices.  Never the one-kernel plan, never a recorded graph; prepared DFT_Fxc* tables (all slots)
 * and later DFT_ComputeXC* results are left bit for bit.  d_ao_hess may be 0 for an LDA-class solver.
 * Returns 0, or -1 with DFT_GetLastError: a null pointer, bad sizes, a null ao_hess on a gradient solver, and "quirks" = 1
 * with vwn5_c or pbe_c in the functional (DFT_ComputeXCSpin's refusal: the potentials are derivatives of the energy).
 * Added without a change of DFT_GetVersion (it stays 5): look the symbol up. */
int DFT_ComputeXCGradientSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr,
                              unsigned long long d_dm_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_weights_ptr,
                              unsigned long long d_ao_grad_ptr, unsigned long long d_ao_hess_ptr,
                              unsigned long long d_out_ptr);

/* XC part of the nuclear gradient of a meta-GGA (csrc/xc_grad_meta.hip), a solver made by DFT_CreateSolverMeta.
 * DFT_ComputeXCGradientMeta: d_out (nao, 3) receives G of the Exc DFT_ComputeXCMeta returns, under DFT_ComputeXCGradient's
 * column replacement (dm and the weights fixed; tau changes through its gradient planes).  With ct = w e_tau / 2 as
 * "xc_points_meta" writes it and Y_k = (d_k AO) Ds,
 *     G[mu, x] = G_gga[mu, x; c0..c3] - 2 sum_g ct sum_k hess_xk[g, mu] Y_k[g, mu]:
 * the six Hessian planes, no third derivatives.  Order of work on the solver's stream: the sweep's density kernels with
 * the sweep's choices into the planes of that set, the padded symmetric matrix, "tau" on it, "xc_points_meta", then the
 * contraction in the form option "xcg_meta_fused" chooses -- 1 (the default: the faster form as measured,
 * profiles/xc_gradient_meta_time.txt): k_xc_grad_meta<true>, one pass over the ten planes with five products per load of
 * the matrix; 0: k_xc_grad on c0..c3 and k_xc_grad_meta<false> (the tau term) into two slab sets
 * and one fixed-order sum over both, the plain form the fused kernel is tested against.  With both meta weights zero the
 * tau stage and the tau term are left out and the result is DFT_ComputeXCGradient's of the same mix.  No atomics: a call
 * is bitwise reproducible.  Asynchronous, never the one-kernel plan, never a recorded graph; its planes, tau, coefficients,
 * padded matrix and slabs are the gradient entries' one set (see DFT_ComputeXCSpin), which no sweep and no prepared table
 * holds, so later DFT_ComputeXCMeta / DFT_ComputeXCGradient / DFT_ComputeXC results and prepared DFT_Fxc* tables are bit for
 * bit what they were.
 * DFT_ComputeXCEnergyDensityMeta: d_e_out (ngrid) receives the energy per volume of the meta point WITHOUT the weight
 * (density stage and "tau" as above, then "xc_edens_meta"): sum_g w_g e_g is DFT_ComputeXCMeta's Exc.
 * Both return 0, or -1 with DFT_GetLastError, before any launch: a solver without meta weights, a null pointer (ao_grad
 * and ao_hess included), bad sizes, "quirks" = 1 with vwn5_c / pbe_c, and a basis whose tiles do not fit 160 KB of LDS
 * (nao above 1216 in the fused form, above 1328 in the plain one, whose k_xc_grad tiles are the wider); several faults in one
 * call: the order stated at DFT_ComputeXCSpin. */
int DFT_ComputeXCGradientMeta(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr,
                              unsigned long long d_ao_ptr, unsigned long long d_weights_ptr,
                              unsigned long long d_ao_grad_ptr, unsigned long long d_ao_hess_ptr,
                              unsigned long long d_out_ptr);
int DFT_ComputeXCEnergyDensityMeta(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr,
                                   unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                                   unsigned long long d_e_out_ptr);

/* The same at two spin densities (csrc/xc_grad_meta_spin.hip): the XC part of the nuclear gradient of an open-shell meta-GGA.
 * DFT_ComputeXCGradientMetaSpin: d_out (nao, 3) receives G of the Exc DFT_ComputeXCMetaSpin returns, under the same column
 * replacement.  With the coefficients of the spin point as "xc_points_meta_spin" writes them (one-sided, ct_s = w e_tau_s / 2),
 * Ds_s the symmetric part of dm_s and Y_sk = (d_k AO) Ds_s,
 *     G[mu, x] = sum_s { G_gga[mu, x; c_s0..c_s3, Ds_s] - 2 sum_g ct_s sum_k hess_xk[g, mu] Y_sk[g, mu] }.
 * Order of work on the solver's stream: the sweep's density kernels once per spin, the padded symmetric matrices, the tau
 * stage of the open-shell sweep on them ("tau_spin", or "tau x2" with option "tau_spin_fused" = 0), "xc_points_meta_spin",
 * then the contraction in the form option "xcg_meta_spin_fused" chooses -- 1 (the default: the faster form as measured,
 * profiles/xc_gradient_meta_spin_time.txt): k_xc_grad_meta_spin, both spins in one pass over the ten planes, six staged
 * tiles and ten products per step on two loads of the matrices; 0: per spin k_xc_grad on c_s0..c_s3 and k_xc_grad_meta<false> (the tau term), four slab sets and one
 * fixed-order sum over them, the plain form the fused kernel is tested against.  With both meta weights zero the tau stage and
 * the tau term are left out and the contraction is DFT_ComputeXCGradientSpin's of the same mix, honouring "xcg_spin_fused".
 * No atomics: a call is bitwise reproducible.  Asynchronous, never the one-kernel plan, never a recorded graph; it works in
 * the gradient entries' one set (see DFT_ComputeXCSpin), so later sweeps, the other gradient-side entries and prepared
 * DFT_Fxc* tables are bit for bit what they were.
 * DFT_ComputeXCEnergyDensityMetaSpin: d_e_out (ngrid) receives the energy per volume of the spin meta point WITHOUT the
 * weight (density stage and "tau" as above, then "xc_edens_meta_spin"; a channel below the density cut-off is absent as in
 * the sweep): sum_g w_g e_g is DFT_ComputeXCMetaSpin's Exc.
 * Both return 0, or -1 with DFT_GetLastError, before any launch: a solver without meta weights, a null pointer (ao_grad
 * and ao_hess included), bad sizes, "quirks" = 1 with vwn5_c / pbe_c, and a basis whose tiles do not fit 160 KB of LDS
 * (nao above 1616 in the fused form, above 1328 in the plain one, whose k_xc_grad tiles are the wider); several faults in one
 * call: the order stated at DFT_ComputeXCSpin. */
int DFT_ComputeXCGradientMetaSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr,
                                  unsigned long long d_dm_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_weights_ptr,
                                  unsigned long long d_ao_grad_ptr, unsigned long long d_ao_hess_ptr,
                                  unsigned long long d_out_ptr);
int DFT_ComputeXCEnergyDensityMetaSpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr,
                                       unsigned long long d_dm_b_ptr, unsigned long long d_ao_ptr,
                                       unsigned long long d_ao_grad_ptr, unsigned long long d_e_out_ptr);

/* Grid response of the nuclear gradient (csrc/becke.hip): what the derivative at fixed points and weights leaves out.
 * With Exc = sum_g w0_g cell_g e_g -- w0 the atomic radial x angular weight, cell_g = P_own(r_g) / sum_C P_C(r_g) the
 * Becke cell function of the point's own atom (three smoothing iterations, radius adjustment a_CD clipped to +-1/2),
 * e_g the energy per volume -- the entries below give e_g and sum_g f_g D_B cell_g for the caller's f_g = w0_g e_g.
 * DFT_ComputeXCEnergyDensity: d_e_out (ngrid) receives e_g of the density of dm, WITHOUT the weight: sum_g w_g e_g is the
 * Exc DFT_ComputeXC returns.  The density kernels of the sweep with the sweep's choices ("path", nao, plane size) into
 * the planes of the gradient entries' set, then "xc_edens": the body the sweep's pointwise kernel runs for the solver's type with unit
 * weight, so the density cut-off, "quirks" and the mix weights are the sweep's.
 * DFT_ComputeXCEnergyDensitySpin: the same of DFT_ComputeXCSpin(dm_a, dm_b): the density kernels on dm_a and on dm_b and
 * the spin-resolved body; it refuses what DFT_ComputeXCSpin refuses ("quirks" = 1 with vwn5_c / pbe_c).
 * Both are asynchronous on the solver's stream, never the one-kernel plan, never a recorded graph; prepared DFT_Fxc*
 * tables (all slots) and later DFT_ComputeXC* results are left bit for bit as they were.  d_ao_grad may be 0 for an
 * LDA-class solver.
 * DFT_BeckeWeightGradient: d_out (natm, 3) receives sum_g f_g D_B cell_g, where D_B cell_g is the derivative of cell_g by
 * R_B at FIXED r_g for B other than the point's owner, and minus the sum of those for the owner (the point moves with its
 * owner and the cell function is translationally invariant), so the rows of d_out sum to zero.  atom_xyz (natm, 3) bohr
 * and atom_radius (natm; the Bragg radius in bohr: a_CD is made of sqrt(radius) as grid_gen.becke_weights makes it) are
 * HOST arrays; d_coords (ngrid, 3) fp64, d_owner (ngrid) int32 in [0, natm) (values outside are clamped, the caller
 * vouches for them), d_f (ngrid) fp64; d_cell_out (ngrid) receives cell_g, or is 0.  "becke_wgrad": a workgroup keeps the
 * distances and the cell functions of a tile of points in LDS -- 64 points up to 60 atoms, 32 up to 120, 16 up to 240, 8
 * beyond -- and every (point, B) pair walks the atoms C once (fp64 vector ALU, O(natm^2) per point, no screening of
 * distant atoms); one (natm, 3) slab per workgroup and a fixed-order slab sum: no floating-point atomics, a call is
 * bitwise reproducible.  No formula divides by a cell function or a switching factor that can be zero; a point on a
 * nucleus is served.  natm above 1005 is refused (the tile no longer fits 160 KB of LDS).  Asynchronous on the solver's
 * stream, except that a call with other atoms than the last one uploads its tables and waits for that.
 * All return 0, or -1 with DFT_GetLastError (nothing aborts): a null pointer, bad sizes, a null ao_grad on a gradient
 * solver, the "quirks" case, a radius that is not positive, coinciding atoms, natm too large.  Added without a change of
 * DFT_GetVersion (it stays 5): look the symbols up. */
int DFT_ComputeXCEnergyDensity(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_ptr,
                               unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr, unsigned long long d_e_out_ptr);
int DFT_ComputeXCEnergyDensitySpin(XCSolver *solver, long long ngrid, int nao, unsigned long long d_dm_a_ptr,
                                   unsigned long long d_dm_b_ptr, unsigned long long d_ao_ptr, unsigned long long d_ao_grad_ptr,
                                   unsigned long long d_e_out_ptr);
int DFT_BeckeWeightGradient(XCSolver *solver, long long ngrid, int natm, const double *atom_xyz, const double *atom_radius,
                            unsigned long long d_coords_ptr, unsigned long long d_owner_ptr, unsigned long long d_f_ptr,
                            unsigned long long d_cell_out_ptr, unsigned long long d_out_ptr);

/* Columns of the electron-repulsion matrix on the device: all (ij|kl) with k in shell C and l in shell D, for every
 * i >= j -- what the integral-direct pivoted Cholesky factorisation of the ERI asks for per pivot (cholesky.py; the
 * reference builds the whole tensor on the host with PySCF, `mol.intor('int2e')` at grid.py:65).  Device counterpart
 * of the host engine's column routine (csrc/integrals.c::qc_eri_cols2: same McMurchie-Davidson formulation, s-f
 * shells, same Schwarz screening).  Shell table as for DFT_EvalAO (host arrays, copied once); qmax_pairs: the Schwarz
 * bounds sqrt(max (ab|ab)) of the nshell (nshell + 1) / 2 shell pairs a >= b in the order a (a + 1) / 2 + b.
 * DFT_EriColumns clears and fills d_out: ((2 l_C + 1)(2 l_D + 1), nao, nao) f64, matrix (k, l) at index
 * k (2 l_D + 1) + l, elements i >= j only (each matrix is symmetric; the other triangle stays zero).  Asynchronous on
 * the handle's stream (default: the null stream).  Returns 0 or -1 (DFT_EriColumnsLastError). */
void *DFT_EriColumnsOpen(int nshell, const double *shl_xyz, const int *shl_l, const int *shl_nprim,
                         const int *shl_off, const int *shl_ao, const double *prim_exp, const double *prim_coef,
                         int nao, int nprim_total, const double *qmax_pairs);
int DFT_EriColumns(void *handle, int shell_C, int shell_D, double screen, unsigned long long d_out_ptr);
/* Several ket shell pairs in one call (their kernels run side by side): block k, laid out as DFT_EriColumns does, starts
 * offsets[k] doubles into d_out; blocks must not overlap, [0, largest end) is cleared as a whole. */
int DFT_EriColumnsMany(void *handle, int npairs, const int *shell_C, const int *shell_D, double screen,
                       unsigned long long d_out_ptr, const long long *offsets);
int DFT_EriColumnsSetStream(void *handle, unsigned long long hip_stream);
const char *DFT_EriColumnsLastError(void *handle);
void DFT_EriColumnsClose(void *handle);

/* One-electron Coulomb integrals at points, A[c][mu][nu] = int phi_mu(r) phi_nu(r) / |r - R_c| dr, contracted on the device
 * without being stored (csrc/point_coulomb.hip; device counterpart of the host engine's qc_point_matrix /
 * qc_point_contract: the McMurchie-Davidson nuclear-attraction integral of csrc/integrals.c::qc_int1e for arbitrary
 * centres, s-f shells).  Shell table as for DFT_EvalAO (host arrays, copied once).  Open returns NULL without a device
 * or for a shell with l > 3.
 *   Matrix    d_out (nao, nao), overwritten: M = sum_c w_c A[c], both triangles, M == M^T bit for bit -- the matrix of
 *             npts point charges w_c at d_points_xyz (npts, 3) bohr, with the sign of A: the external potential of
 *             charges q in Hcore is -M(q).  Sums over points in a fixed order, no atomics: the same bits every run.
 *   Contract  d_out (npts), overwritten: u[c] = sum_{mu nu} D[mu][nu] A[c][mu][nu] for any (nao, nao) matrix D (it need
 *             not be symmetric); for a density matrix the electronic part of the electrostatic potential is -u.
 *   Field     d_out (npts, 3), overwritten: G[c][k] = sum_{mu nu} D[mu][nu] dA[c][mu][nu] / dR_c,k, k = x, y, z -- the
 *             gradient of Contract's u with respect to the point (exact: the basis does not move with the point).  For a
 *             density matrix the electronic part of the electric field is +G.  Same arguments, error returns and
 *             determinism as Contract.  Added without a change of DFT_GetVersion (it stays 5): a caller that may meet an
 *             older library detects this entry by looking the symbol up (dlsym), not by the version.
 * npts is 64-bit; npts == 0 is valid (Matrix writes zeros, Contract and Field write nothing).  Asynchronous on the handle's
 * stream (default: the null stream); every entry runs on the device that was current at Open.  Returns 0 or -1
 * (DFT_PointCoulombLastError); nothing aborts. */
void *DFT_PointCoulombOpen(int nshell, const double *shl_xyz, const int *shl_l, const int *shl_nprim,
                           const int *shl_off, const int *shl_ao, const double *prim_exp, const double *prim_coef,
                           int nao, int nprim_total);
int DFT_PointCoulombMatrix(void *handle, long long npts, unsigned long long d_points_xyz, unsigned long long d_weights,
                           unsigned long long d_out);
int DFT_PointCoulombContract(void *handle, long long npts, unsigned long long d_points_xyz, unsigned long long d_dm,
                             unsigned long long d_out);
int DFT_PointCoulombField(void *handle, long long npts, unsigned long long d_points_xyz, unsigned long long d_dm,
                          unsigned long long d_out);
int DFT_PointCoulombSetStream(void *handle, unsigned long long hip_stream);
const char *DFT_PointCoulombLastError(void *handle);
void DFT_PointCoulombClose(void *handle);

/* The two-electron term of the nuclear gradient, contracted on the device as the derivative integrals are made
 * (csrc/grad2e.hip; device counterpart of the host engine's qc_grad2e / grad_quartet, s-f shells, the dense ERI never
 * built).  Shell table as for DFT_EvalAO (host arrays, copied once).  Open returns NULL without a device, for a shell
 * with l > 3 or a shell table that does not fit nao / nprim_total.
 *   d_dm   (nao, nao) f64 on the device, symmetric (only then is the result the derivative below).
 *   d_out  (nshell, 3) f64 on the device, overwritten:
 *            out[A][x] = d/dR_A,x of  1/2 sum_abcd D_ab D_cd (ab|cd) - c_hf/4 sum_abcd D_ac D_bd (ab|cd),
 *          the derivative acting on the functions of shell A in the FIRST index only, times the 4 equivalent positions
 *          -- element-wise: sum over shells B and ket pairs C >= D of
 *            sum_{a in A, b in B, c in C, d in D} [2 f D_ab D_cd - c_hf (D_ac D_bd + (C != D) D_ad D_bc)] d(ab|cd)/dA_x,
 *          f = 1 for C == D and 2 otherwise.  The rows of an atom's shells add up to the atom's gradient term.
 * Every primitive pair with |c_a c_b| exp(-mu R^2) < 1e-18 is dropped, as on the host; nothing else is screened.  Partial
 * sums are added in a fixed order, no floating-point atomics: the same call twice gives the same bits.  Asynchronous on
 * the handle's stream (default: the null stream).  DFT_Grad2e and SetStream return 0, or -1 for a null handle or
 * pointer, a refused LDS request or a failed launch (DFT_Grad2eLastError); nothing aborts.  Added without a change of
 * DFT_GetVersion (it stays 5): look the symbols up. */
void *DFT_Grad2eOpen(int nshell, const double *shl_xyz, const int *shl_l, const int *shl_nprim, const int *shl_off,
                     const int *shl_ao, const double *prim_exp, const double *prim_coef, int nao, int nprim_total);
int DFT_Grad2e(void *handle, unsigned long long d_dm, double c_hf, unsigned long long d_out);
/* The same for an open-shell state, in one pass over the derivative integrals: d_dm the total density D = D_a + D_b,
 * d_ms the spin density M = D_a - D_b (both (nao, nao) f64 on the device, symmetric), and
 *   out[A][x] = d/dR_A,x of  1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum (D_ac D_bd + M_ac M_bd) (ab|cd)
 * in DFT_Grad2e's element-wise conventions: the density quartet is
 *   2 f D_ab D_cd - c_hf [D_ac D_bd + M_ac M_bd + (C != D)(D_ad D_bc + M_ad M_bc)].
 * Only the gather of the density quartet differs from DFT_Grad2e; the handle's tables, streams and partial sums are
 * shared, so the two entries may alternate on one handle and each stays bitwise reproducible.  Asynchronous on the
 * handle's stream.  Returns 0, or -1 (DFT_Grad2eLastError) under DFT_Grad2e's conditions and for a null d_ms. */
int DFT_Grad2eSpin(void *handle, unsigned long long d_dm, unsigned long long d_ms, double c_hf, unsigned long long d_out);
int DFT_Grad2eSetStream(void *handle, unsigned long long hip_stream);
const char *DFT_Grad2eLastError(void *handle);
void DFT_Grad2eClose(void *handle);

/* The rest of an SCF cycle on the device: between the cycle's J / K / Vxc and the next density the
 * reference's loop runs on the host -- Fock assembly (dft.py:212-223), Pulay DIIS (dft.py:225), eigh(F, S) (dft.py:227),
 * dm = 2 C_occ C_occ^T (dft.py:228) and the energy traces (dft.py:231-234).  DFT_ScfTailStep queues all of it behind
 * the kernels that produced J, K and Vxc (csrc/scf_tail.hip): the eigenproblem as the occupied-subspace rotation of
 * scf.OccupiedRotation from the basis in d_basis.  For 2 <= nao <= 512, 1 <= nocc <= 64 (NULL from Open otherwise; up to
 * 128 x 32 the rotation's matrices live in LDS, above in memory).
 *   Open    hcore, overlap: (nao, nao) device, read in every step; d_basis: (nao, nao) device, columns = an
 *           S-orthonormal basis whose first nocc columns span the occupied space (the eigenvectors of the last full
 *           diagonalisation, uploaded by the caller; replaced by the rotated basis after every successful step);
 *           d_fock_out: (nao, nao) device, receives the DIIS-extrapolated Fock matrix of every step; d_mo_energy:
 *           nao doubles or 0 (occupied: exact levels of the rotated block, virtual: diagonal estimates).
 *   Step    rotate = 0: DIIS only (status 1).  c_hf: exact-exchange fraction (K may be 0).  tol: residual at which the
 *           rotation's fixed point stops; canon_tol: the Jacobi sweeps that make the occupied block diagonal end with
 *           the first sweep that met no column pair with |cos| above it (the pairs are then below ~canon_tol^2;
 *           <= 0: 1e-3); max_inner: fixed-point steps allowed (<= 0: 60).  slot: ring slot (0..7) that
 *           receives this cycle's (F, e); hist: the nhist <= 8 live slots, `slot` among them; coef: NULL, or the nhist
 *           Pulay coefficients to use instead of solving for them.  d_J, d_K, d_vraw: this cycle's matrices (vraw as
 *           DFT_ComputeXC leaves it: symmetrised here, dft.py:212); d_dm (nao, nao), d_cocc (nao, nocc) with
 *           dm = cocc cocc^T: the CURRENT density in, the NEXT one out (status 0 only).  d_exc: 0, or the device scalar
 *           a DFT_ComputeXC*Async call queued before this step writes: Wait then returns it as out[7], and the whole
 *           cycle needs one host wait.
 *   Finish  after status 1: the caller has diagonalised d_fock_out and put the eigenvectors into d_basis; writes
 *           cocc = sqrt(2) basis[:, :nocc], dm and the traces.
 *   Wait    blocks (polling host-mapped memory) until the last Step / Finish has completed; out[0..6] = tr(dm' Hcore),
 *           tr(dm' J)/2, -c_hf tr(dm' K)/4, |dm' - dm|_F, status, fixed-point steps, Jacobi sweeps, Exc (see d_exc).  status 0: done;
 *           1: diagonalise d_fock_out yourself, then Finish; 2: the DIIS system was singular (DFT_ScfTailGram copies the
 *           8 x 8 Gram matrix of the ring to the host: solve it there and repeat the Step with `coef`); 3: see DFT_ScfTailMore.
 * Everything is asynchronous on the handle's stream except Wait and Gram.  0 on success, -1 on error. */
void *DFT_ScfTailOpen(int nao, int nocc, unsigned long long d_hcore, unsigned long long d_overlap, unsigned long long d_basis,
                      unsigned long long d_fock_out, unsigned long long d_mo_energy);
int DFT_ScfTailSetStream(void *handle, unsigned long long hip_stream);
int DFT_ScfTailStep(void *handle, int rotate, double c_hf, double tol, double canon_tol, int max_inner, int slot, int nhist,
                    const int *hist, const double *coef, unsigned long long d_J, unsigned long long d_K,
                    unsigned long long d_vraw, unsigned long long d_dm, unsigned long long d_cocc, unsigned long long d_exc);
int DFT_ScfTailFinish(void *handle, double c_hf, unsigned long long d_J, unsigned long long d_K, unsigned long long d_dm,
                      unsigned long long d_cocc);
/* Above 128 functions / 32 occupied orbitals the rotation's fixed-point steps are launches of their own, queued in advance
 * (SetStepsHint: how many per Step, 1..60, default 6); status 3 from Wait = they were not enough: More queues `nsteps` more and
 * the rest of the step again (same matrices as the Step it continues), then Wait again. */
int DFT_ScfTailMore(void *handle, int nsteps, unsigned long long d_J, unsigned long long d_K, unsigned long long d_dm,
                    unsigned long long d_cocc, unsigned long long d_exc);
int DFT_ScfTailSetStepsHint(void *handle, int nsteps);
int DFT_ScfTailWait(void *handle, double *out8);
int DFT_ScfTailGram(void *handle, double *host_out64);
int DFT_ScfTailStamps(void *handle, long long *host_out16);   /* diagnostics: 100 MHz stamps of the rotation kernel's phases */
const char *DFT_ScfTailLastError(void *handle);
void DFT_ScfTailClose(void *handle);

/* Options: "quirks" (1 = reference formulas as shipped, default; 0 = corrected
 * VWN5 / PBE-c derivatives), "path" (0 = auto: wave-specialised
 * persistent MFMA kernels for nao <= 128, generic MFMA kernels above; 1 =
 * plain-VALU validation kernels; 2 = generic MFMA kernels always), "profile"
 * (1 = record per-kernel HIP events for DFT_GetTimings), "ksplit" (grid chunks
 * of the generic Vxc contraction; 0 = auto), "spin_wait" (1, default: the host
 * polls the host-mapped Exc word written by the last kernel instead of sleeping
 * in hipStreamSynchronize), "fuse_finish" (0, default; 1 = the Vxc reduce kernel publishes Exc itself, one launch
 * fewer: DFT_ComputeXC may then return while that kernel's last blocks still store Vxc, which only
 * consumers on the solver's own stream are ordered behind), "strict_sync" (with fuse_finish = 1: 1 =
 * DFT_ComputeXC also waits for the stream to report complete before returning), "occ" (DFT_ComputeXCOcc:
 * 0 = auto, 1 = always the occupied-orbital density step, 2 = never), "dm_factor" (DFT_ComputeXC / DFT_ComputeXC64,
 * which receive a dm and no orbitals: 0 = never, the default; 1 = try: with path = 0, outside the "tiny" plan and with
 * occ != 2, dm is factorised as by DFT_FactorDensity (default max_rank and tol) into a workspace of the solver, and where
 * it is accepted AND the "occ" rule takes the occupied form at that rank, the sweep runs as DFT_ComputeXCOcc does with the
 * factor as cocc; in every other case the call runs exactly as with 0, the same kernels and the same bits.  Such a call is
 * neither recorded nor replayed as a graph.  The asynchronous entries, DFT_ComputeXCOcc* and DFT_ComputeXCDirect ignore
 * the option.  Its initial value is 1 when the environment variable QCDFT_DM_FACTOR is "1" at DFT_CreateSolver /
 * DFT_CreateSolverMix -- the variable is sampled once, there: how an unmodified caller of the four reference symbols
 * opts in), "eri_symmetric" (0, default: DFT_ComputeCoulomb is
 * eri^T . vec(dm) for any matrix, the reference's GEMV; 1 = the caller vouches that eri is symmetric as an (nao^2, nao^2)
 * matrix, (ij|kl) = (kl|ij), as every real ERI is: only its upper triangle is read, half the bytes and half the time; 2 = ... and
 * in each index pair, (ij|kl) = (ji|kl) = (ij|lk), and dm = dm^T: only the unique eighth is read, 51 against 240 us at Benzene/def2-SVP; below 48 functions both values keep the full pass), "graph" (the synchronous calls: -1 = auto, default:
 * a call repeated with the same pointers and sizes is replayed as one recorded HIP graph where it is launch-bound,
 * planes of at most 2e6 doubles; 1 = always; 0 = never.  Same kernels, same results bit for bit), "tiny" (bases of at most 32 functions: -1 = auto, default: the
 * whole sweep -- density, functional, Vxc contraction of a 16-point sub-tile -- in ONE kernel plus the slab sum where that is
 * the faster call, which it is at every size measured (0.71-1.00 of the four launches, 20 k-300 k points: profiles/r03_tiny_scan_final.txt);
 * 1 = whenever nao <= 32; 0 = never.  Results agree with the four-launch path to the
 * rounding of the sums, not bit for bit.  A SOLVER_MIX solver never takes it, whatever the option says: the one-pass
 * kernel is register-critical and instantiated for the three built-in bodies only, so a mix runs the general kernels at
 * every nao), "ao_pt" (grid points per workgroup of DFT_EvalAO:
 * 8, 16, or 0 = auto), "vxc_fringe" (the wave-specialised Vxc kernel at nao = 16 k + 1..4, k >= 1, every solver type but
 * B3LYP: -1 = auto and 1: the matrix cores take the k x k whole tiles and one wave adds the 1..4 fringe lines on the vector
 * ALU, instead of padding to k + 1 tiles per side; 0 = the padded kernel.  Same slabs, Vxc equal to the rounding of the
 * fringe sums, Exc bit for bit), "publish" (how the synchronous calls learn that the sweep has completed, with
 * fuse_finish = 0: 0 = a one-thread kernel behind the Vxc reduce copies Exc to the host-mapped word; 1 = the reduce kernel
 * stores Exc there itself and a stream memory write (hipStreamWriteValue64) behind it raises a per-call sequence word
 * the host waits for -- same contract, no launch; taken only where a probe at DFT_CreateSolver found the runtime
 * performs the operation, else the kernel stays; -1 = auto, default: the kernel, which measured 1-2 us faster per call.
 * A recorded graph always ends with the kernel), "xcg_spin_fused" (DFT_ComputeXCGradientSpin: 1, default = both spins in
 * one k_xc_grad launch; 0 = k_xc_grad once per spin, the plain form the tests hold it to), "xcg_meta_fused"
 * (DFT_ComputeXCGradientMeta: 1, default = k_xc_grad_meta<true>, one pass, the faster form as measured; 0 = k_xc_grad and
 * the tau-term kernel, the plain form the tests hold it to), "xcg_meta_spin_fused" (DFT_ComputeXCGradientMetaSpin: 1, default =
 * k_xc_grad_meta_spin, both spins in one pass, the faster form as measured; 0 = the plain pair once per spin, the form the
 * tests hold it to).
 * Returns 0 if the key is known. */
int DFT_SetOption(XCSolver *solver, const char *key, double value);

/* Read-back of "publish", "vxc_fringe", "fuse_finish", "strict_sync", "spin_wait", "graph", "tiny", "sweep_order", "path",
 * "quirks", "occ", "dm_factor", and of what the library made of them: "used_occ" (1 = the last sweep took the
 * occupied-orbital density step), "used_dm_factor" (1 = the last synchronous call swept with the factor of its dm),
 * "dm_factor_rank" (the rank its attempt found; 0 = rejected, or nothing was attempted), "publish_probe" (1 = the creation-time probe of the stream memory
 * write passed), "publish_live" (1 = a synchronous call now completes by stream write), "used_publish" and
 * "used_vxc_fringe" (what the last synchronous call / the last sweep did).  NaN for an unknown key.  Added without a
 * change of DFT_GetVersion: a caller that may meet an older library looks the symbol up. */
double DFT_GetOption(XCSolver *solver, const char *key);

/* Run subsequent work on `hip_stream` (a hipStream_t cast to an integer);
 * 0 restores the null stream. */
int DFT_SetStream(XCSolver *solver, unsigned long long hip_stream);

/* Last error text ("" if none).  The pointer stays valid until the next call
 * on the same solver. */
const char *DFT_GetLastError(XCSolver *solver);

/* With option "profile"=1: durations (ms) of the kernels of the last
 * DFT_ComputeXC* call (with option "dm_factor": "dm_factor" and "dm_factor_check" in front) or of the last
 * DFT_FactorDensity, DFT_FxcPrepare ("rho" or "rho_occ", "fxc_table"), DFT_FxcPrepareSpin (the same with
 * "fxc_table_spin"), DFT_FxcApply / DFT_FxcApplyKind ("rho", "fxc_coef", "fxc_vxc",
 * "fxc_reduce") or DFT_ComputeXCSpin ("rho" for alpha, "rho" for beta, "xc_points_spin", "fxc_vxc" and
 * "fxc_reduce" for alpha -- the contraction without an energy --, "vxc" and "reduce_vxc" for beta), DFT_FxcPrepareSpinPol ("rho", "rho", "fxc_table_pol") or DFT_FxcApplySpinPol ("rho", "rho",
 * "fxc_coef_pol", then "fxc_vxc", "fxc_reduce" twice), in launch order; names[i] (if non-NULL) receives a
 * static string.  Returns the number of entries written (<= max_entries). */
int DFT_GetTimings(XCSolver *solver, double *ms, const char **names, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* QCDFT_AMD_DFT_SOLVER_H */
