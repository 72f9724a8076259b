// pba_internal.h -- engine entry points shared by the engine and the host LM driver (not part of the public ABI).
#pragma once
#include "../../include/pba.h"

extern "C" {
// grad_only != 0: stop after the reduced solve (cost / gradient norms of the linearisation point only).  scal: nullptr, or 32 doubles
// for the step's raw scalar block (pba_lm_rules.h: Scal), which PBA_ERR_NUMERIC fills too.
int pba_internal_step(pba_engine* e, double radius, int32_t init_scale, const pba_solver_options* o, pba_step_info* out, double* scal,
                      int grad_only);
int pba_internal_ready(pba_engine* e);   /* PBA_OK, or PBA_ERR_STATE with the reason in pba_last_error */
int pba_internal_world(const pba_engine* e);
int pba_internal_rank(const pba_engine* e);
int pba_internal_is_multi(const pba_engine* e);   /* collectives are enqueued with every step */
int64_t pba_internal_local_blocks(const pba_engine* e);
int pba_internal_patch_len(const pba_engine* e);
// pose-only mode (pba_set_points_constant): on / residual blocks of the reduced program (all of them outside the mode) / cost of the
// constant camera's residual blocks as the last step found it (0 outside the mode) / sets pba_last_error and returns `code`
int pba_internal_points_constant(const pba_engine* e);
int64_t pba_internal_program_blocks(const pba_engine* e);
void pba_internal_covariance_times(const pba_engine* e, double* ms4);      // event time of the kernels of the last pba_covariance
void pba_internal_marginal_times(const pba_engine* e, double* ms5);        // event time of the kernels of the last pba_marginalize
// test hook: the radix-select kernels of pba_cull on a caller's array; *out = the k-th smallest of v [n] (0-based) by 64-bit pattern
int pba_internal_select_u64order(pba_engine* e, const double* v, int64_t n, int64_t k, double* out);
double pba_internal_fixed_cost(const pba_engine* e);
int pba_internal_refuse(pba_engine* e, int code, const char* msg);
int pba_internal_allreduce_host(pba_engine* e, double* v, int n, int op);
// candidate pass = Jacobian pass (speculative linearisation) on/off
void pba_internal_set_speculate(pba_engine* e, int on);
void pba_internal_pass_counts(const pba_engine* e, int64_t* jac, int64_t* cost);
void pba_internal_reset_pass_counts(pba_engine* e);
// asynchronous driver (device-side trust-region decisions)
int pba_internal_async_capable(const pba_engine* e, const pba_solver_options* o);
int pba_internal_async_begin(pba_engine* e, const pba_solver_options* o);
int pba_internal_async_enqueue(pba_engine* e, int kind, int init_scale, const pba_solver_options* o, unsigned long long* seq_out);
int pba_internal_async_wait(pba_engine* e, unsigned long long seq);
const void* pba_internal_async_state(const pba_engine* e);
const pba_iteration_summary* pba_internal_async_log(const pba_engine* e);
int pba_internal_async_end(pba_engine* e);
// resident solve (pba_resident.h): the whole pba_solve as ONE cooperative launch
int pba_internal_resident_capable(pba_engine* e, const pba_solver_options* o);
/* PBA_INTERNAL_RESIDENT_REFUSED: the runtime refused the cooperative launch before anything ran -- nothing changed, the engine has left the
   resident driver for good and the caller runs the solve on the pipelined one */
#define PBA_INTERNAL_RESIDENT_REFUSED (-1000)
int pba_internal_resident_launch(pba_engine* e, const pba_solver_options* o, unsigned long long* seq_out);
void pba_internal_resident_done(pba_engine* e, int iterations);   /* the solve took `iterations` step trips: unused epochs go back */
void pba_internal_resident_failed(pba_engine* e);   /* a resident launch ended without publishing (device-side wait timed out): the engine is unusable */
void pba_internal_resident_trace(pba_engine* e, int iterations);   /* PBA_RES_TRACE: phase intervals of the last resident solve to stderr */
int pba_internal_final_flushes(const pba_engine* e);   /* 1: the kind-2 enqueue also flushes (no kind 3 behind it) */
// batched solves (pba_solve_batch, pba_batch.h): validate (nothing touches a device), begin (streams ordered and lent, every window begun,
// the window table uploaded), one batched pass of kind 0 | 1 | 2 over the windows sel[] (indices into es), end (streams given back)
int pba_internal_batch_validate(pba_engine* const* es, int32_t n, const pba_solver_options* o);
int pba_internal_batch_begin(pba_engine* const* es, int32_t n, const pba_solver_options* o);
int pba_internal_batch_enqueue(pba_engine* const* es, const int32_t* sel, int32_t n_sel, int kind, int init_scale, unsigned long long* seq_out);
void pba_internal_batch_end(pba_engine* const* es, int32_t n, int failed);
}
