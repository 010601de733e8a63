// The C ABI of the MI355X kernel library: every exported entry point, declared exactly once.
//
// pdt_common.h includes this header, so every translation unit sees every declaration: a
// definition that disagrees with its declaration is a compile error ("conflicting types"), and
// a call across translation units needs no local copy of the prototype. The Python layer reads
// this same file (ops/native_ops.py) and derives its ctypes argument and result types from it.
//
// Plain declarations only, `PDT_API <ret> name(<params>);`, grouped by the source file that
// defines them, over a closed set of types: int, long, unsigned, float, double, hipStream_t and
// pointers to void / float / int / long / int64_t (const or not). What an argument means is
// documented at its definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PDT_API extern "C" __attribute__((visibility("default")))

// attention.hip
PDT_API int pdt_attn_set_bwd_single(int on);
PDT_API int pdt_attn_set_tiled(int on);
PDT_API int pdt_attn_fwd(const void* qkv, void* out, float* lse, int B, int T, int H, float scale, hipStream_t st);
PDT_API int pdt_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                         void* dqkv, int B, int T, int H, float scale, hipStream_t st);
PDT_API int pdt_attn_bwd_q8(const void* qkv, const void* out, const void* dout, const float* lse, float* delta,
                            void* dqkv, int B, int T, int H, float scale, void* q8, float* q8_meta, float* q8_part,
                            float* q8_dq, hipStream_t st);

// attention_bwd_f8.hip
PDT_API int pdt_attn_bwd_f8_grid(int B, int H);
PDT_API int pdt_attn_bwd_f8_q8(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                               int B, int T, int H, float scale, void* q8, const float* q8_meta, float* q8_part,
                               float* q8_dq, float* colpart, float* bias_out, hipStream_t st);
PDT_API int pdt_attn_bwd_f8(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B,
                            int T, int H, float scale, hipStream_t st);
PDT_API int pdt_attn_bwd_f8_debug(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                  int B, int T, int H, float scale, float* dbg, hipStream_t st);

// attention_cls.hip
PDT_API int pdt_cls_attn_fwd(const void* qkv, void* o, float* lse, int B, int T, int H, hipStream_t st);
PDT_API int pdt_cls_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv, int B,
                             int T, int H, hipStream_t st);

// attention_f8.hip
PDT_API int pdt_attn_set_pv8(int on);
PDT_API int pdt_attn_fwd_f8(const void* qkv, void* out, float* lse, int B, int T, int H, float scale, hipStream_t st);
PDT_API int pdt_attn_fwd_f8_q8(const void* qkv, void* out, float* lse, int B, int T, int H, float scale, void* q8,
                               float* q8_meta, float* q8_part, float* q8_dq, hipStream_t st);
PDT_API int pdt_attn_fwd_tiles(const void* qkv, void* out, float* lse, int B, int T, int H, float scale,
                               hipStream_t st);

// bn_act.hip
PDT_API int pdt_bn_stats_blocks(long M, int C);
PDT_API long pdt_rows_reduce_workspace(int R, int C);
PDT_API int pdt_bn_finalize(const float* part, int R, int C, double count, float eps, float momentum,
                            const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                            float* shift, float* running_mean, float* running_var, long* num_batches_tracked,
                            hipStream_t st);
PDT_API int pdt_bn_apply(const void* y, const void* res, void* out, const float* scale, const float* shift, long M,
                         int C, int relu, void* mask, hipStream_t st);
PDT_API int pdt_bn_apply_res_affine(const void* y, const void* r, void* out, const float* scale, const float* shift,
                                    const float* rscale, const float* rshift, long M, int C, int relu, void* mask,
                                    hipStream_t st);
PDT_API int pdt_bn_bwd_reduce(const void* dA, const void* y, const void* act, const float* mean, const float* scale,
                              const float* shift, float* part, long M, int C, int relu, int blocks, const void* mask,
                              hipStream_t st);
PDT_API int pdt_bn_bwd_finalize(const float* part, int R, int C, double count, const float* gamma, const float* mean,
                                const float* invstd, float* dgamma, float* dbeta, float* k1, float* k2, float* k3,
                                int accumulate, hipStream_t st);
PDT_API int pdt_bn_bwd_apply_dual(const void* dA, const void* mask, const void* y1, const float* k1a,
                                  const float* k2a, const float* k3a, void* dy1, const void* y2, const float* k1b,
                                  const float* k2b, const float* k3b, void* dy2, long M, int C, hipStream_t st);
PDT_API int pdt_bn_bwd_apply(const void* dA, const void* y, const void* act, const float* scale, const float* shift,
                             const float* k1, const float* k2, const float* k3, void* dy, void* dres, long M, int C,
                             int relu, const void* mask, hipStream_t st);
PDT_API int pdt_bn_bwd_reduce_pool(const void* dout, const void* idx, const void* y, const float* mean,
                                   const float* scale, const float* shift, float* part, int N, int H, int W, int C,
                                   int Ho, int Wo, int k, int s, int p, int blocks, hipStream_t st);
PDT_API int pdt_bn_bwd_apply_pool(const void* dout, const void* idx, const void* y, const float* scale,
                                  const float* shift, const float* k1, const float* k2, const float* k3, void* dy,
                                  int N, int H, int W, int C, int Ho, int Wo, int k, int s, int p, hipStream_t st);

// conv_igemm.hip
PDT_API int pdt_conv_nt_num_variants();
PDT_API int pdt_conv_nt_variant_kind(int v);
PDT_API int pdt_conv_nt_resolve_variant(int variant, int M, int Ncol, int K);
PDT_API int pdt_conv_nt_bnb_rows(int M, int Ncol, int K, int variant);
PDT_API int pdt_conv_nt_bnb_supports(int variant, int has_addend, int has_mask, int relu, int two);
PDT_API int pdt_conv_nt_stat_rows(int M, int Ncol, int K, int variant);
PDT_API int pdt_conv_nt(const void* src, const void* b, void* out, float* stats, const float* bias,
                        const void* addend, const void* addend_mask, int Hs, int Ws, int Cs, int Nimg, int Hm, int Wm,
                        int Ncol, int K, int ldb, int sh, int sw, int oh0, int ow0, int dh, int dw, int nth, int ntw,
                        int Ho, int Wo, int osh, int osw, int oph, int opw, int ldo, int act, void* aux, int variant,
                        int pix, hipStream_t stream);
PDT_API int pdt_conv_nt_bnb(const void* src, const void* b, void* out, const void* addend, const void* addend_mask,
                            int Hs, int Ws, int Cs, int Nimg, int Hm, int Wm, int Ncol, int K, int ldb, int sh,
                            int sw, int oh0, int ow0, int dh, int dw, int nth, int ntw, int Ho, int Wo, int osh,
                            int osw, int oph, int opw, int ldo, int variant, const void* bn_y, const float* bn_mean,
                            const float* bn_scale, const float* bn_shift, const void* bn_mask, float* part, int relu,
                            int row0, int R, hipStream_t stream);
PDT_API int pdt_conv_nt_bnb2(const void* src, const void* b, void* out, const void* addend, const void* addend_mask,
                             int Hs, int Ws, int Cs, int Nimg, int Hm, int Wm, int Ncol, int K, int ldb, int sh,
                             int sw, int oh0, int ow0, int dh, int dw, int nth, int ntw, int Ho, int Wo, int osh,
                             int osw, int oph, int opw, int ldo, int variant, const void* bn_y, const float* bn_mean,
                             const float* bn_scale, const float* bn_shift, const void* bn_mask, float* part, int relu,
                             int row0, int R, const void* bn_y2, const float* bn_mean2, float* part2,
                             hipStream_t stream);
PDT_API int pdt_conv_nt_ax3(const void* src, const void* b, void* out, float* stats, const void* addend,
                            const void* addend_mask, int Hs, int Ws, int Cs, int Nimg, int Hm, int Wm, int Ncol,
                            int K, int ldb, int sh, int sw, int oh0, int ow0, int dh, int dw, int nth, int ntw,
                            int Ho, int Wo, int osh, int osw, int oph, int opw, int ldo, int variant,
                            const void* bn_y, const float* bn_mean, const float* bn_scale, const float* bn_shift,
                            const void* bn_mask, float* part, int relu, int row0, int R, int ax_mode,
                            const void* ax_y2, const float* ax_c1, const float* ax_c2, const float* ax_c3,
                            const float* ax_rsc, const float* ax_rsh, const void* ax_mask_in, void* ax_mask_out,
                            void* ax_dst, hipStream_t stream);
PDT_API int pdt_conv_nt_ax(const void* src, const void* b, void* out, float* stats, int Hs, int Ws, int Cs, int Nimg,
                           int Hm, int Wm, int Ncol, int K, int ldb, int ldo, int variant, const void* bn_y,
                           const float* bn_mean, const float* bn_scale, const float* bn_shift, const void* bn_mask,
                           float* part, int relu, int row0, int R, int ax_mode, const void* ax_y2, const float* ax_c1,
                           const float* ax_c2, const float* ax_c3, const float* ax_rsc, const float* ax_rsh,
                           const void* ax_mask_in, void* ax_mask_out, void* ax_dst, hipStream_t stream);
PDT_API int pdt_gemm_f8_num_variants();
PDT_API int pdt_gemm_f8(const void* a, const void* b, void* out, const float* bias, const float* dq_a,
                        const float* dq_b, int M, int N, int K, int lda, int ldb, int ldo, int fmt_a, int act,
                        void* aux, const void* addend, int variant, hipStream_t stream);
PDT_API int pdt_gemm_f8_bm(int variant);
PDT_API long pdt_gemm_f8_q8_part(int M, int N);
PDT_API int pdt_gemm_f8_q8(const void* a, const void* b, void* out, const float* bias, const float* dq_a,
                           const float* dq_b, int M, int N, int K, int lda, int ldb, int ldo, int fmt_a, int act,
                           void* aux, const void* addend, int variant, void* q8, float* q8_meta, float* q8_part,
                           int q8_fmt, int q8_only, float* q8_dq, hipStream_t stream);
PDT_API int pdt_gemm_f8_q8_cs(const void* a, const void* b, void* out, const float* bias, const float* dq_a,
                              const float* dq_b, int M, int N, int K, int lda, int ldb, int ldo, int fmt_a, int act,
                              void* aux, const void* addend, int variant, void* q8, float* q8_meta, float* q8_part,
                              int q8_fmt, int q8_only, float* q8_dq, float* colsum, hipStream_t stream);

// conv_wgrad.hip
PDT_API int pdt_wgrad_num_variants();
PDT_API int pdt_wgrad_halo_id();
PDT_API int pdt_wgrad_plan2(int M, int Mo, int No, int Hs, int Ws, int C, int variant, int* per_split);
PDT_API long pdt_wgrad_workspace(int splits, int Mo, int No);
PDT_API int pdt_conv_wgrad2(const void* dy, const void* x, float* slab, float* out, int M, int Mo, int No, int ldy,
                            int Hs, int Ws, int C, int Hm, int Wm, int sh, int sw, int oh0, int ow0, int dh, int dw,
                            int ntw, int splits, int ktiles_per_split, float scale, int accumulate, int variant,
                            int pix, float* bias_out, const void* bn_y, const float* bn_c, hipStream_t stream);
PDT_API long pdt_reduce_rows_work(int nrows, int n);
PDT_API int pdt_wgrad_reduce_rows(const float* rows, float* out, int nrows, int n, float scale, int accumulate,
                                  float* work, hipStream_t stream);
PDT_API int pdt_wgrad_reduce(float* slab, float* out, const float* bslab, float* bias_out, int splits, int Mo, int No,
                             float scale, int accumulate, hipStream_t stream);

// drop_path.hip
PDT_API int pdt_drop_path_scales(float* scale, int* state, const float* p, const float* inv_keep, int n_branches,
                                 int B, long sample0, hipStream_t st);

// ema.hip
PDT_API int pdt_ema_update(const void* chunks, int nchunks, void* ema, const void* src, void* shadows, float* dev,
                           float decay, int warmup, hipStream_t st);

// eval_stats.hip (ks: nk <= 8 ints in HOST memory; loss_sum / counts are added to)
PDT_API int pdt_eval_stats(const void* logits, int bf16, long ld, const long* target, int kind, float eps,
                           const int* ks, int nk, float* loss_rows, int* rank, double* loss_sum, long* counts, int B,
                           int V, hipStream_t st);

// fp8.hip
PDT_API int pdt_amax_blocks(long n);
PDT_API int pdt_amax_partial(const void* x, int bf16, long n, float* partial, hipStream_t st);
PDT_API int pdt_cast_fp8(const void* x, int bf16, long n, const float* partial, int fmt, void* q, float* dq,
                         hipStream_t st);
PDT_API int pdt_cast_fp8_dual(const float* x, int R, int C, const float* partial, void* q, void* qt, float* dq,
                              hipStream_t st);
PDT_API int pdt_fp8_meta_words();
PDT_API int pdt_cast_fp8_delayed(const void* x, int bf16, long n, float* meta, int fmt, void* q, float* dq_out,
                                 hipStream_t st);
PDT_API int pdt_gelu_dual_cast_fp8(const void* y, long n, float* meta, int fmt, void* q, void* aux, void* a_out,
                                   float* dq_out, hipStream_t st);
PDT_API int pdt_cast_cs_bands(int rows);
PDT_API int pdt_cast_fp8_delayed_cs(const void* x, int rows, int cols, float* meta, int fmt, void* q, float* dq_out,
                                    float* cpart, float* bias_out, hipStream_t st);
PDT_API int pdt_cast_fp8_gelu_grad_cs(const void* x, const void* z, int rows, int cols, float* meta, int fmt, void* q,
                                      float* dq_out, float* cpart, float* bias_out, hipStream_t st);
PDT_API int pdt_fp8_meta_roll_partial(float* meta, const float* partial, int nblk, int fmt, float* dq_out,
                                      hipStream_t st);
PDT_API int pdt_fp8_meta_seed(const float* partial, long n, int fmt, float* meta, hipStream_t st);

// gemm_ring.hip
PDT_API int pdt_gemm_ring_num_variants();
PDT_API int pdt_gemm_ring_grid(int M, int N, int sub);
PDT_API int pdt_gemm_ring_bm();
PDT_API int pdt_gemm_ring(const void* a, const void* b, void* c, const float* bias, const float* dq_a,
                          const float* dq_b, int M, int N, int K, int lda, int ldb, int ldc, int dt, int sub,
                          hipStream_t st);
PDT_API int pdt_gemm_ring_epi(const void* a, const void* b, void* c, const float* bias, const float* dq_a,
                              const float* dq_b, int M, int N, int K, int lda, int ldb, int ldc, int dt, int act,
                              void* aux, const void* addend, void* q8, const float* q8_meta, float* q8_part,
                              int q8_fmt, int q8_only, float* colsum, hipStream_t st);
PDT_API int pdt_gemm_ring_epi_pers(const void* a, const void* b, void* c, const float* bias, const float* dq_a,
                                   const float* dq_b, int M, int N, int K, int lda, int ldb, int ldc, int dt, int act,
                                   void* aux, const void* addend, void* q8, const float* q8_meta, float* q8_part,
                                   int q8_fmt, int q8_only, float* colsum, hipStream_t st);

// image_aug.hip
PDT_API int pdt_crop_resize_norm_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box,
                                         void* out, long B, int S, int Cp, const float* mean, const float* inv_std,
                                         hipStream_t st);
PDT_API int pdt_crop_resize_norm_mix_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box,
                                             const int64_t* pidx, const int* pbox, const int* rect,
                                             const float* w_own, void* out, long B, int S, int Cp, const float* mean,
                                             const float* inv_std, hipStream_t st);
PDT_API int pdt_crop_resize_norm_erase_u8_bf16(const void* src, int Hs, int Ws, const int64_t* idx, const int* box,
                                               const int64_t* pidx, const int* pbox, const int* rect,
                                               const float* w_own, const int* erect, int R, const void* ekey,
                                               int emode, void* out, long B, int S, int Cp, const float* mean,
                                               const float* inv_std, hipStream_t st);

// layernorm.hip
PDT_API int pdt_ln_fwd(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, int rows,
                       int D, float eps, hipStream_t st);
PDT_API int pdt_ln_fwd_f8_blocks(int rows);
PDT_API int pdt_ln_add_fwd(const void* x, const void* r, void* xsum, const float* g, const float* b, void* y,
                           float* mean, float* rstd, int rows, int D, float eps, void* q, float* meta,
                           float* amax_part, float* dq_out, hipStream_t st);
PDT_API int pdt_ln_add_dp_fwd(const void* x, const void* r, void* xsum, const float* g, const float* b, void* y,
                              float* mean, float* rstd, int rows, int D, float eps, void* q, float* meta,
                              float* amax_part, float* dq_out, const float* scale, int rows_per_sample,
                              hipStream_t st);
PDT_API int pdt_ln_fwd_f8(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, int rows,
                          int D, float eps, void* q, float* meta, float* amax_part, float* dq_out, hipStream_t st);
PDT_API int pdt_ln_bwd_blocks(int rows);
PDT_API int pdt_ln_bwd(const void* dy, const void* x, const float* g, const float* mean, const float* rstd, void* dx,
                       float* dg, float* db, float* part, int rows, int D, int accumulate, const void* addend,
                       hipStream_t st);
PDT_API int pdt_ln_bwd_f8(const void* dy, const void* x, const float* g, const float* mean, const float* rstd,
                          void* dx, float* dg, float* db, float* part, int rows, int D, int accumulate,
                          const void* addend, void* q8, float* q8_meta, float* q8_part, float* q8_dq, hipStream_t st);
PDT_API int pdt_ln_bwd_f8_db(const void* dy, const void* x, const float* g, const float* mean, const float* rstd,
                             void* dx, float* dg, float* db, float* part, int rows, int D, int accumulate,
                             const void* addend, void* q8, float* q8_meta, float* q8_part, float* q8_dq, float* cpart,
                             float* bias_out, int bias_acc, hipStream_t st);
PDT_API int pdt_ln_dp_bwd(const void* dy, const void* x, const float* g, const float* mean, const float* rstd,
                          void* dx, void* dyb, float* dg, float* db, float* part, int rows, int D, int accumulate,
                          const void* addend, const float* scale, int rows_per_sample, void* q8, float* q8_meta,
                          float* q8_part, float* q8_dq, float* cpart, float* bias_out, int bias_acc,
                          hipStream_t st);
PDT_API int pdt_gelu_bwd(const void* dy, const void* z, void* dz, long n, hipStream_t st);

// lenet.hip
PDT_API int pdt_lenet_grad_row(int nc);
PDT_API int pdt_lenet_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* wf1, const float* bf1, const float* wf2, const float* bf2, int B, int NC,
                          int training, float p2, float p1, unsigned seed, float* logp, void* mask2, void* mask1,
                          hipStream_t st);
PDT_API int pdt_lenet_bwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* wf1, const float* bf1, const float* wf2, const float* bf2, int B, int NC,
                          int training, float p2, float p1, unsigned seed, const float* dlogp, float* part,
                          float* grads, hipStream_t st);
PDT_API int pdt_nll_fwd(const float* logp, const int64_t* tgt, int B, int C, int ignore, float* loss, float* count,
                        float* bad, hipStream_t st);
PDT_API int pdt_nll_bwd(const int64_t* tgt, const float* g, const float* count, int B, int C, int ignore,
                        float* dlogp, hipStream_t st);

// misc.hip
PDT_API int pdt_fill_uniform_bf16(void* out, long n, unsigned seed, hipStream_t st);
PDT_API int pdt_synth_images_bf16(void* out, const int64_t* idx, long B, int HW, int C, int Cp, unsigned seed,
                                  int64_t* labels, int classes, hipStream_t st);
PDT_API int pdt_cast_f32_bf16(const float* x, void* y, long n, hipStream_t st);
PDT_API int pdt_wt_dgrad(const float* w, void* out, int Cout, int KH, int KW, int Cin, int kh0, int kw0, int s,
                         int nth, int ntw, hipStream_t st);
PDT_API int pdt_wt_job_size();
PDT_API int pdt_wt_dgrad_multi(const void* jobs, int njobs, long total, hipStream_t st);
PDT_API int pdt_transpose_cast(const float* w, void* out, int R, int C, hipStream_t st);
PDT_API int pdt_lane_reduce_probe(const float* x, float* out, int n, hipStream_t st);

// optim.hip
PDT_API int pdt_chunk_struct_size();
PDT_API int pdt_sgd_step2(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          float lr, float momentum, float dampening, float wd, int nesterov, int first,
                          float grad_scale, const float* dev, hipStream_t st);
PDT_API int pdt_adam_step2(const void* chunks, int nchunks, void* params, const void* grads, void* exp_avg,
                           void* exp_avg_sq, void* max_sq, void* shadows, float lr, float b1, float b2, float eps,
                           float wd, int decoupled, float bc1, float bc2, float grad_scale, float* dev, int tick,
                           hipStream_t st);
PDT_API int pdt_sgd_step3(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          float lr, float momentum, float dampening, float wd, int nesterov, int first,
                          float grad_scale, const float* dev, const float* glob, int skip_nonfinite, int* skipped,
                          hipStream_t st);
PDT_API int pdt_adam_step3(const void* chunks, int nchunks, void* params, const void* grads, void* exp_avg,
                           void* exp_avg_sq, void* max_sq, void* shadows, float lr, float b1, float b2, float eps,
                           float wd, int decoupled, float bc1, float bc2, float grad_scale, float* dev, int tick,
                           const float* glob, int skip_nonfinite, int* skipped, hipStream_t st);

// optim_layerwise.hip
PDT_API int pdt_sumsq_chunks(const void* chunks, int nchunks, const void* a, const void* b, float* partials,
                             hipStream_t st);
PDT_API int pdt_norm_finalize(const float* partials, const int* chunk_begin, int n_tensors, int nroles, int grole,
                              float* norms, float* glob, int start_zero, float max_grad_norm, hipStream_t st);
PDT_API int pdt_lars_step(const void* chunks, int nchunks, void* params, const void* grads, void* bufs, void* shadows,
                          const int* flags, const float* norms, int n_tensors, const float* glob, float lr,
                          float momentum, float wd, int nesterov, float trust, float eps, const float* dev,
                          hipStream_t st);
PDT_API int pdt_lamb_tick(float* dev, double b1, double b2, hipStream_t st);
PDT_API int pdt_lamb_stage1(const void* chunks, int nchunks, const void* params, const void* grads, void* exp_avg,
                            void* exp_avg_sq, const int* flags, float* partials, const float* glob, float b1,
                            float b2, float omb1, float omb2, float eps, float wd, float bc1, float bc2,
                            const float* dev, hipStream_t st);
PDT_API int pdt_lamb_stage2(const void* chunks, int nchunks, void* params, const void* exp_avg,
                            const void* exp_avg_sq, void* shadows, const int* flags, const float* norms,
                            int n_tensors, float lr, float eps, float wd, float bc1, float bc2, const float* dev,
                            hipStream_t st);

// pool.hip
PDT_API int pdt_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int Ho, int Wo, int k,
                            int s, int p, hipStream_t st);
PDT_API int pdt_maxpool_fwd_affine(const void* x, void* y, void* idx, const float* scale, const float* shift, int N,
                                   int H, int W, int C, int Ho, int Wo, int k, int s, int p, hipStream_t st);
PDT_API int pdt_maxpool_bwd(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, int Ho, int Wo,
                            int k, int s, int p, hipStream_t st);
PDT_API int pdt_avgpool_fwd(const void* x, void* y, int N, int HW, int C, hipStream_t st);
PDT_API int pdt_avgpool_bwd(const void* dy, void* dx, int N, int HW, int C, hipStream_t st);
PDT_API int pdt_maxpool_bwd_bnred(const void* dy, const void* idx, void* dx, const void* y, const float* mean,
                                  const float* scale, const float* shift, float* part, int N, int H, int W, int C,
                                  int Ho, int Wo, int blocks, hipStream_t st);

// stem.hip
PDT_API int pdt_stem_fwd_rows(int N, int H, int W, int Cout);
PDT_API int pdt_stem_fwd(const void* x4, const void* w256, void* y, float* part, int N, int H, int W, int Cout,
                         hipStream_t stream);
PDT_API int pdt_stem_wgrad_splits_v(int N, int H, int W, int Cout, int variant);
PDT_API int pdt_stem_wgrad_v(const void* x4, const void* dA, const void* y, const float* bnc, float* slab, int N,
                             int H, int W, int Cout, int variant, hipStream_t stream);

// wgrad_f8.hip
PDT_API int pdt_wgrad_f8_num_variants();
PDT_API int pdt_wgrad_f8_plan(int M, int Mo, int No, int variant, int* ktiles_per_split);
PDT_API long pdt_wgrad_f8_workspace(int splits, int Mo, int No);
PDT_API int pdt_linear_wgrad_f8(const void* dy8, const void* x8, const float* dq_dy, const float* dq_x,
                                const void* dy16, float* slab, float* out, float* bias_out, int M, int Mo, int No,
                                int ldy, int ldx, int splits, int ktiles_per_split, int accumulate, int variant,
                                hipStream_t stream);

// wgrad_ring.hip
PDT_API int pdt_wgrad_ring_ok(int Mo, int No, int C, int pix);
PDT_API int pdt_wgrad_ring_launch(const void* dy, const void* x, float* slab, int M, int Mo, int No, int ldy, int Hs,
                                  int Ws, int C, int Hm, int Wm, int sh, int sw, int oh0, int ow0, int dh, int dw,
                                  int ntw, int splits, int ktiles_per_split, int pix, hipStream_t st);

// xent.hip
PDT_API int pdt_xent_fwd(const void* logits, int bf16, const long* target, float* lse, float* loss_rows,
                         float* loss_out, int B, int V, float eps, hipStream_t st);
PDT_API int pdt_xent_bwd(const void* logits, int bf16, const long* target, const float* lse, const float* gout,
                         void* dlogits, int B, int V, float eps, hipStream_t st);
PDT_API int pdt_xent_pair_fwd(const void* logits, int bf16, const long* ta, const long* tb, const float* lam,
                              float* lse, float* loss_rows, float* loss_out, int B, int V, float eps,
                              hipStream_t st);
PDT_API int pdt_xent_pair_bwd(const void* logits, int bf16, const long* ta, const long* tb, const float* lam,
                              const float* lse, const float* gout, void* dlogits, int B, int V, float eps,
                              hipStream_t st);
PDT_API long pdt_colsum_workspace(int R, int C);
PDT_API int pdt_colsum(const void* x, float* out, float* work, int R, int C, int acc, hipStream_t st);
