/* muse_lbfgs.h -- libmuse_lbfgs.so: lock-step L-BFGS / HagerZhang for a batch of problems whose objective is the CALLER's
 * (reverse communication: the objective of every problem is evaluated by the caller, once per round for the whole batch; everything
 * between two evaluations -- the directional derivative, the line search's state machine, acceptance, the convergence tests, the
 * history update, the two-loop recursion, the next trial point -- runs for all problems in one kernel launch, one workgroup per
 * problem).  The algorithm is optim.lbfgs of the Python package decision for decision (Optim.jl's LBFGS(m = 10) with
 * LineSearches' InitialStatic(1) and HagerZhang defaults); only the order of summation inside a dot product differs.
 *
 * A library of its own, apart from libmuse_hip.so (include/muse_hip.h), with no context and no state: all state lives in a workspace
 * the caller allocates on the device.  No entry point allocates, synchronises or reads the device; every launch goes to `stream`
 * (a hipStream_t; NULL: the default stream), so the calls order with the caller's own work on that stream.  Because nothing is read
 * back, the batch's shape (nprob, n, m) is an argument of every call; it must be the same from begin to result.
 *
 *     bytes = muse_lbfgs_workspace_bytes(nprob, n, m);                  ws: that many bytes of device memory, 256-byte aligned
 *     muse_lbfgs_begin(ws, nprob, n, m, z0, g_tol, maxiter, z_eval, stream);
 *     do {
 *         f[b], g[b][:] = objective and gradient of problem b at z_eval[b][:]          (the caller's, for every b)
 *         muse_lbfgs_advance(ws, nprob, n, m, f, g, z_eval, active, stream);
 *         synchronise the stream
 *     } while (*active > 0);
 *     muse_lbfgs_result(ws, nprob, n, m, z_out, info_out, stream);
 *
 * z0, z_eval, g, z_out: [nprob][n] doubles in device memory, dense rows (stride n; any 8-byte alignment).  f: [nprob] doubles in
 * device memory.  A problem's result depends on its own inputs only: not on the batch, nor on its place in it.  A finished
 * problem's z_eval row stays at its final point (the objective keeps seeing finite input), its record no longer changes and the
 * values passed for it are ignored.
 *
 * A second reverse-communication solver of the same build: lock-step CONJUGATE GRADIENTS for a batch of rows, each one linear system
 * M y = b with M symmetric positive definite and APPLIED BY THE CALLER (get_H! by implicit differentiation for closure problems: M is
 * minus the Hessian of logLike in z at a simulation's MAP, a double backward pass of the caller's closure; one row per simulation and
 * column).  Once per round the caller evaluates M p for all rows as one [nrows][n] batch; everything between two evaluations -- p.Mp,
 * the guard, the updates of y and r, r.r, the stopping rule, the next direction -- is one launch, one workgroup per row.  Plain CG from
 * y = 0 in the order of IterativeSolvers' cg without a preconditioner; a row stops at |r|_2 <= max(reltol |b|_2, abstol) (the
 * recurrence residual) or after maxiter iterations.
 *
 *     bytes = muse_lbfgs_cg_workspace_bytes(nrows, n);                  ws: that many bytes of device memory, 256-byte aligned
 *     muse_lbfgs_cg_begin(ws, nrows, n, b, reltol, abstol, maxiter, p_eval, active, stream);      synchronise the stream
 *     while (*active > 0) {
 *         Mp[r][:] = M_r p_eval[r][:]                                                  (the caller's, for every row r)
 *         muse_lbfgs_cg_advance(ws, nrows, n, Mp, p_eval, active, stream);
 *         synchronise the stream
 *     }
 *     muse_lbfgs_cg_result(ws, nrows, n, y_out, iterations_out, resnorm_out, stream);
 *
 * b, p_eval, Mp, y_out: [nrows][n] doubles in device memory, dense rows as above; p_eval overlaps neither b nor Mp.  The direction p
 * lives in p_eval and nowhere else: the caller must leave it as the library wrote it.  The same contract: no state but the workspace,
 * nothing allocates, synchronises or reads the device, the shape is an argument of every call, a row's result depends on its own
 * inputs and n only.  A finished row's p_eval row stays where it is (the operator keeps seeing finite input) and what is passed for it
 * is ignored.  A row whose p.Mp is not positive or not finite -- M is not positive definite there -- stops with y as it was and the
 * count -1 - iterations (include/muse_hip.h's convention for the implicit get_H!).
 *
 * The same solver with a DIAGONAL (Jacobi) preconditioner Pl = Diagonal(d), in the order of IterativeSolvers' preconditioned cg: the
 * number of rounds is the cost of a solve (every round is one application of the caller's operator, one launch and one
 * synchronisation), and a preconditioner is the only lever on it.  muse_lbfgs_pcg_begin / muse_lbfgs_pcg_advance take the place of
 * muse_lbfgs_cg_begin / muse_lbfgs_cg_advance in the loop above; the workspace (muse_lbfgs_cg_workspace_bytes: r / d is formed where it
 * is used and never stored) and muse_lbfgs_cg_result are shared, and a workspace may be used for one kind of solve after the other.
 * diag: [nrows / rows_per_diag][n] doubles in device memory, the caller's, the same from begin to the last advance; row r reads
 * diagonal row r / rows_per_diag (get_H!: the columns of one simulation share one Hessian, so its diagonal is held once).  The first
 * direction is b / d; the stopping rule is plain CG's, on |r|_2.  Any diagonal of positive finite entries gives the same solution to
 * the tolerance -- only the count moves; a row whose diagonal holds an entry that is not positive or not finite is stopped in begin
 * with y = 0 and the count -1 (its p_eval row is b), unless it needs no iteration at all (count 0, as in plain CG).  With d = 1 every
 * value is plain CG's.
 *
 * Every function returns 0, or a negative number: MUSE_LBFGS_BAD_ARGUMENT, or -(100 + the hipError_t of a failed launch).
 */
#ifndef MUSE_LBFGS_H
#define MUSE_LBFGS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUSE_LBFGS_M 10                /* the history length: the only value of m the library accepts */
#define MUSE_LBFGS_BAD_ARGUMENT (-1)

/* the workspace's size in bytes (negative: a bad argument) */
int64_t muse_lbfgs_workspace_bytes(int64_t nprob, int64_t n, int m);

/* start nprob problems at z0 with gradient tolerance g_tol and at most maxiter iterations; writes the first evaluation point (z0
 * itself) into z_eval */
int muse_lbfgs_begin(void* ws, int64_t nprob, int64_t n, int m, const double* z0, double g_tol, int maxiter, double* z_eval, void* stream);

/* one round: consumes f and g at z_eval, writes the next z_eval row of every active problem, and stores the number of problems
 * still active to *active_out -- one int, in pinned host memory (or any memory the device can write); valid once the stream has
 * reached this point */
int muse_lbfgs_advance(void* ws, int64_t nprob, int64_t n, int m, const double* f, const double* g, double* z_eval, int* active_out,
                       void* stream);

/* the minimisers z_out [nprob][n] and one record per problem in info_out (device memory), in the layout of muse_hip.h's solver info:
 * int32 iterations, f_calls, status, hist_words (0); double f_min, gnorm.  status: 0 g_converged, 1 x_converged, 2 f_converged,
 * 3 maxiter, 4 linesearch_failed, 5 nonfinite */
int muse_lbfgs_result(void* ws, int64_t nprob, int64_t n, int m, double* z_out, void* info_out, void* stream);

/* the advance kernel's workgroup size for rows of length n (a function of n alone) */
int muse_lbfgs_workgroup_size(int64_t n);

/* ---- lock-step conjugate gradients (the shape limits and the workgroup size are those above) ---- */

/* the workspace's size in bytes: one record per row and [nrows][2][n] doubles, y and r (negative: a bad argument); the same for the
 * preconditioned solver */
int64_t muse_lbfgs_cg_workspace_bytes(int64_t nrows, int64_t n);

/* start nrows systems with right-hand sides b: y = 0, r = b, the first direction (b itself) into p_eval, the tolerance
 * max(reltol |b|, abstol); a row with b = 0 (or within abstol) or maxiter == 0 is finished at once with count 0.  *active_out as for
 * muse_lbfgs_advance */
int muse_lbfgs_cg_begin(void* ws, int64_t nrows, int64_t n, const double* b, double reltol, double abstol, int maxiter, double* p_eval,
                        int* active_out, void* stream);

/* one round: consumes Mp = M p_eval, writes the next direction of every active row into p_eval and the number of rows still active to
 * *active_out */
int muse_lbfgs_cg_advance(void* ws, int64_t nrows, int64_t n, const double* Mp, double* p_eval, int* active_out, void* stream);

/* the solutions y_out [nrows][n], the counts iterations_out [nrows] (int32; negative: -1 - iterations, the guard stopped the row) and
 * resnorm_out [nrows], the recurrence residual |r|_2 (all device memory) */
int muse_lbfgs_cg_result(void* ws, int64_t nrows, int64_t n, double* y_out, int32_t* iterations_out, double* resnorm_out, void* stream);

/* muse_lbfgs_cg_begin with the preconditioner Diagonal(diag): y = 0, r = b, the first direction b / d into p_eval.  diag is
 * [nrows / rows_per_diag][n]; a bad argument also: a null diag, rows_per_diag < 1, nrows not a multiple of rows_per_diag.  A row whose
 * diagonal holds an entry that is not positive or not finite is finished with the count -1 and b in its p_eval row */
int muse_lbfgs_pcg_begin(void* ws, int64_t nrows, int64_t n, const double* b, const double* diag, int64_t rows_per_diag, double reltol,
                         double abstol, int maxiter, double* p_eval, int* active_out, void* stream);

/* muse_lbfgs_cg_advance for a solve begun by muse_lbfgs_pcg_begin, with the same diag and rows_per_diag */
int muse_lbfgs_pcg_advance(void* ws, int64_t nrows, int64_t n, const double* Mp, const double* diag, int64_t rows_per_diag, double* p_eval,
                           int* active_out, void* stream);

/* ---- the engine's normal stream, for all rows of a map in one launch ----
 *
 * The stream of (seed, sim) is the engine's (include/muse_hip.h; csrc/rng.hpp): Philox4x32-10 keyed by the seed with the counter
 * (element, sim), and a fixed-sequence Box-Muller that gives element i the pair (n1(i), n2(i)) = normal_pair(seed, sim, i).  As a
 * SEQUENCE e_0, e_1, ... it is
 *
 *     e_{2i} = n1(i),   e_{2i+1} = n2(i).
 *
 * A request for k values returns the next k values and starts at a pair boundary: the cursor, counted in pairs, advances by
 * ceil(k / 2), and an odd request discards its last n2.  The stream is a pure function of (seed, sim, i) -- it is never advanced by
 * the library; the cursor is the caller's, passed as pair_offset -- so a simulation's numbers are the same alone or in any batch,
 * and bit-equal to what the engine gives that simulation's elements.
 *
 * out[r][j] = e_{2*pair_offset + j} of stream (seed, sims[r]) for j < count.
 * out: [nrows][count] doubles in device memory, dense rows (stride count; any 8-byte alignment).  sims: [nrows] int64 in device
 * memory, every one non-negative (the package's MASTER_SIM = 2^62 - 1 and DATA_SIM = 2^32 - 1 included).  A bad argument: a null out
 * or sims, nrows < 1, count < 1, pair_offset < 0, nrows * ceil(count / 2048) above 2^31 - 1, pair_offset + ceil(count / 2) above
 * 2^63 - 1.  The same contract as above: no state, no allocation, no synchronisation, no read of the device; one launch, to `stream`. */
int muse_lbfgs_normals(double* out, int64_t nrows, int64_t count, uint64_t seed, const int64_t* sims, int64_t pair_offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif
