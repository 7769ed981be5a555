// group.h -- internal interface between the BCM layer (bcm.cpp) and the evaluation engine (cugp_capi.cpp, group.cpp, predict.cpp):
// several experts of equal shape on one device evaluated by ONE sequence of launches (blockIdx.y = expert).
// Not part of the public boundary (include/cugp.h).
#pragma once
#include "../../include/cugp.h"

struct cugp_group;

// Scratch of doubles that only grows (the allocations cost more than the kernels using it): device memory, or pinned host
// memory when `pinned`.  grow() first synchronises `stream` (hipStream_t; none when null), which may still read the old
// buffer; a failed allocation leaves {nullptr, 0} and returns CUGP_ERR_NOMEM / CUGP_ERR_DEVICE (cugp_last_error).
struct Scratch {
    double* p = nullptr;
    size_t cap = 0;                  // in doubles
    bool pinned = false;
    int grow(size_t count, void* stream);
    void release();
};

extern "C" {

// experts must live on one device and agree in padded size, dimension and kernel kind, and be all ARD or all isotropic
// (else CUGP_ERR_INVALID)
int cugp_group_create(cugp_gp* const* experts, int k, cugp_group** out);
// cugp_create_ard with the matrices padded to at least npad_min rows (cugp_create_padded's rule): the experts of an ARD BCM
int cugp_create_ard_padded(int n, int d, int device, int npad_min, cugp_gp** out);
void cugp_group_destroy(cugp_group* gr);
// cugp_append refuses an expert of a cugp_bcm (marked here by bcm.cpp, for good) and a handle that a live cugp_group holds
// (counted by cugp_group_create / cugp_group_destroy, which the experts must outlive)
int cugp_mark_bcm_expert(cugp_gp* gp);

// Evaluate all experts at their (common) hyper-parameters; ll[k], g[nh k .. nh k + nh - 1] with nh = 3, or the handles' nh (ARD d + 2, rational quadratic d + 3 or 4)
// experts (g may be null when !want_grad).
// Returns CUGP_ERR_INVALID without touching anything when the experts cannot be evaluated as a group right now
// (different hyper-parameters, profiling on, missing data): the caller then evaluates them one by one.
int cugp_group_eval(cugp_group* gr, int want_grad, double* ll, double* g);
// the same in two halves, so the groups of several devices are all in flight before the first result is read
int cugp_group_enqueue(cugp_group* gr, int want_grad);
int cugp_group_fetch(cugp_group* gr, double* ll, double* g);
// device copy of the results of the evaluation in flight ([k][8] doubles: LL, g0, g1, g2, ...; ARD experts: [k][8 + nh],
// LL at 0, the gradient from entry 8) and the stream
// (hipStream_t) they are ordered on -- for a reduction that stays on the device (RCCL all-reduce)
int cugp_group_device_results(cugp_group* gr, const double** dout, void** stream);
// 4 doubles device -> device on `stream` (hipStream_t); the result row of the evaluation a single expert has in flight
int cugp_copy_device_row(double* dst, const double* src, void* stream);
// [count][4] <- {LL, g0, g1, g2} of every [8]-double result row of src (a group's device results), one 2D copy on `stream`
int cugp_pack_result_rows(double* dst, const double* src, int count, void* stream);
// [count][1 + nh] <- {LL, g[nh]}: the call above for isotropic rows (nh = 3), ARD rows ([8 + nh]) by two 2D copies
int cugp_pack_result_rows_n(double* dst, const double* src, int count, int nh, int ard, void* stream);
// error text for cugp_last_error from the other translation units; returns `code`
int cugp_internal_fail(int code, const char* what);
// halves of cugp_bcm_loglik_grad_allgather (comm.cpp; defined in bcm.cpp)
// (dsend: [local expert][1 + nh], nh = the BCM's)
int cugp_bcm_enqueue_rows_packed(cugp_bcm* b, double* dsend, void** stream);
int cugp_bcm_nh(const cugp_bcm* b);              // 3, d + 2 for an ARD BCM, d + 3 or 4 for a rational quadratic one; 0 for null
int cugp_bcm_is_ard(const cugp_bcm* b);
int cugp_bcm_finish_rows(cugp_bcm* b);
// {LL, g0, g1, g2} of the evaluation a single expert has in flight -> dst (device), on the expert's stream (an ARD
// expert: {LL, g[nh]}, 1 + nh doubles)
int cugp_copy_result_row(cugp_gp* gp, double* dst);
// cugp_predict_cov without the copy to the host (tools/pred_joint_probe.py times the device part with it): Sigma is
// computed, the handle's stream is waited for, and *dcov / *ld give the device matrix (lower tiles valid, row-major,
// leading dimension *ld), which stays valid until the next joint call on the handle
int cugp_predict_cov_device(cugp_gp* gp, const double* Xt, int nt, int with_noise, const double** dcov, int* ld);
// the handle holds L^-1, K^-1, alpha for its current data and hyper-parameters (what a prediction needs)
int cugp_has_inverse(const cugp_gp* gp);
// prediction in two halves, so that the experts of a BCM are all in flight before the first result is read: enqueue
// builds the cross-covariance, its product with L^-T and the means / variances on the handle's stream and copies them
// into `host_mv` (2 * nt doubles, PINNED: mean then variance) behind it; fetch waits for that stream.  The handle must
// hold its inverse quantities (cugp_has_inverse), or enqueue evaluates them first like cugp_predict.
int cugp_predict_enqueue(cugp_gp* gp, const double* Xt, int nt, double* host_mv);
int cugp_predict_fetch(cugp_gp* gp);

// ---- product-of-experts prediction across ranks (cugp_bcm_predict_allgather, comm.cpp) ----
// Rows of the exchange, left on the device: expert i's 1/v at drows[i * row_stride + t], m/v at [i * row_stride + nt + t].
// group: one sequence of batched launches on the lead expert's stream (*stream); CUGP_ERR_INVALID without touching anything
// when the experts cannot predict as a group right now (the caller then enqueues them one by one)
int cugp_group_predict_enqueue(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride, void** stream);
// one expert on its own stream (*stream); cugp_predict_fetch waits for it
int cugp_predict_rows_enqueue(cugp_gp* gp, const double* Xt, int nt, double* drows, void** stream);
// the BCM's side: every local expert's rows into dsend (slot i at dsend + i * slot_stride, slots of 2 nt doubles) with
// `wait_stream` (hipStream_t) ordered behind all of them by events -- no host wait.  Stale experts are brought up to date
// by one cugp_bcm_loglik_grad first.  Only a BCM whose experts are on `device` (else CUGP_ERR_INVALID).
int cugp_bcm_predict_rows_enqueue(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend, size_t slot_stride,
                                  void* wait_stream);
// waits for every local expert's stream (after the rows were used, or after a failed enqueue)
int cugp_bcm_predict_rows_finish(cugp_bcm* b);
// k_poe_reduce on `stream`: gathered [world][rstride] -> dout [mean nt | var nt | world x {status, count}]
int cugp_poe_reduce_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, double* dout,
                            void* stream);

// ---- combination rules on latent rows (cugp_bcm_predict_mode, cugp_bcm_predict_allgather_mode) ----
// The _form twins of the row producers above: latent == 0 is the call above, the same launches and bits; latent != 0 runs
// the same launches with noise_var = 0 in k_predict_finish's by-value scalars, so an expert's rows are 1/var_f and
// m/var_f (var_f = sf2 - |W_t|^2, computed directly).  Layout, batching, passes (tuning key 19) and scratch unchanged.
int cugp_predict_enqueue_form(cugp_gp* gp, const double* Xt, int nt, double* host_mv, int latent);
int cugp_predict_rows_enqueue_form(cugp_gp* gp, const double* Xt, int nt, double* drows, void** stream, int latent);
int cugp_group_predict_enqueue_form(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride,
                                    void** stream, int latent);
int cugp_bcm_predict_rows_enqueue_form(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend,
                                       size_t slot_stride, void* wait_stream, int latent);
// k_poe_reduce_mode on `stream`: cugp_poe_reduce_enqueue's buffers, the rows latent, rule `mode` (CUGP_COMBINE_*)
int cugp_poe_reduce_mode_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, int mode,
                                 double sf2, double sn2, int with_noise, double* dout, void* stream);

// ---- test-input gradients of a product of experts (cugp_bcm_predict_grad, cugp_bcm_predict_grad_allgather) ----
// Rows of one expert, on the device: [m nt | v nt | dmean nt d | dvar nt d], (2 + 2 d) nt doubles; m, v carry cugp_predict's
// bits (latent != 0: cugp_predict_latent's); want_dvar == 0 skips V = W L^-1 and leaves the dvar part untouched.
// (No caller passes want_dvar == 0 today: cugp_bcm_predict_grad and the form across ranks need every expert's dvar for
// the combined MEAN's gradient in every mode.  In the group form that branch -- the gradient launch with V null, the
// finish with dvar null -- has so far run only in the host emulation, tools/bcm_predict_grad_host_check.py; the
// per-expert form's is cugp_predict_grad's own with dvar NULL.)
// group: ONE sequence of batched launches on the lead expert's stream (*stream), expert i's rows at drows + i *
// row_stride; preconditions and contract of cugp_group_predict_enqueue_form -- CUGP_ERR_INVALID without touching anything
// when the experts cannot run as a group right now (the caller then goes expert by expert)
int cugp_group_predict_grad_enqueue(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride,
                                    void** stream, int latent, int want_dvar);
// one expert by cugp_predict_grad's own launches on its own stream (*stream), no host wait; cugp_predict_fetch waits
int cugp_predict_grad_rows_enqueue(cugp_gp* gp, const double* Xt, int nt, double* drows, void** stream, int latent,
                                   int want_dvar);
// the BCM's side of the form across ranks: cugp_bcm_predict_rows_enqueue_form with gradient rows (slots of (2 + 2 d) nt)
int cugp_bcm_predict_grad_rows_enqueue(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend,
                                       size_t slot_stride, void* wait_stream, int latent, int want_dvar);
int cugp_bcm_dim(const cugp_bcm* b);             // the input dimension; 0 for null
// k_poe_reduce_grad on `stream`: gathered [world][rstride] -> dout [mean nt | var nt | dmean nt d | dvar nt d | world x
// {status, count}]; mode CUGP_COMBINE_REFERENCE .. CUGP_COMBINE_RBCM
int cugp_poe_reduce_grad_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, int d, int mode,
                                 double sf2, double sn2, int with_noise, int want_dvar, double* dout, void* stream);
// sf2 = exp(2 theta_f), sn2 = exp(2 theta_n) of the BCM's shared hyper-parameters, as the experts' kernels take them
int cugp_bcm_prior_scalars(const cugp_bcm* b, double* sf2, double* sn2);
}  // extern "C"
