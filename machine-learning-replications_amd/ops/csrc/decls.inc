// Op registry: one HFENS_OP(name, (signature)) line per host entry point.
// Included twice by bindings.cpp: once to declare, once to register with pybind11.
#if defined(HFENS_DECLS)
#define HFENS_OP(name, sig) void name sig;
#elif defined(HFENS_DEFS)
#define HFENS_OP(name, sig) m.def(#name, &hfens::name);
#endif
HFENS_OP(gbdt_apply_prep, (int B, int n, int F, int NN, uintptr_t bins, uintptr_t y, uintptr_t w,
                           uintptr_t raw, uintptr_t g, uintptr_t h, uintptr_t node, uintptr_t prev_feat,
                           uintptr_t prev_blo, uintptr_t prev_value, uintptr_t prev_r2,
                           uintptr_t dev_acc, uintptr_t cur_r2, double lr, double qscale,
                           double dscale, uintptr_t wt, double subsample, uintptr_t seeds,
                           long long row_off, int stage, uintptr_t stream))
HFENS_OP(gbdt_hist, (int B, int n, int F, uintptr_t bins, uintptr_t nbins, int max_nb, uintptr_t g,
                     uintptr_t h, uintptr_t w, uintptr_t node, int node0, int NL, uintptr_t hist,
                     double qscale, uintptr_t stream))
HFENS_OP(gbdt_split, (int B, int F, int NN, uintptr_t hist, uintptr_t nbins, uintptr_t lo_val,
                      uintptr_t hi_val, int node0, int NL, int last_level, double min_leaf_q,
                      double min_split_q, double qscale, uintptr_t feat, uintptr_t blo, uintptr_t thr,
                      uintptr_t value, uintptr_t stats, uintptr_t r2, uintptr_t stream))
HFENS_OP(gbdt_route, (int B, int n, int NN, uintptr_t bins, uintptr_t g, uintptr_t w, uintptr_t node,
                      uintptr_t feat, uintptr_t blo, uintptr_t r2, int node0, int NL, double qscale,
                      uintptr_t stream))
HFENS_OP(gbdt_stumps_fused, (int B, int n, int F, int T, uintptr_t bins, uintptr_t nbins, int hist_len,
                             uintptr_t lo_val, uintptr_t hi_val, uintptr_t y, uintptr_t w, uintptr_t raw,
                             uintptr_t g, uintptr_t h, uintptr_t wt, uintptr_t seeds, long long row_off,
                             double subsample, uintptr_t feat, uintptr_t blo, uintptr_t thr, uintptr_t value,
                             uintptr_t stats, uintptr_t r2, uintptr_t dev, uintptr_t bagw, double lr,
                             double qscale, double dscale, double min_leaf_q, double min_split_q,
                             uintptr_t stream))
HFENS_OP(l1_qp_cd, (int B, int F1, uintptr_t H, uintptr_t g, uintptr_t w, uintptr_t penal, double lam,
                    int max_sweeps, double tol, uintptr_t d_out, uintptr_t stream))
HFENS_OP(logreg_fused, (int B, int n, int F1, uintptr_t X, uintptr_t s, uintptr_t ypm, uintptr_t penal, double C,
                        int l1, int max_outer, uintptr_t Z, uintptr_t Xd, uintptr_t W, uintptr_t iters,
                        uintptr_t stream))
HFENS_OP(logreg_coop, (int B, int members, int n, int F1, uintptr_t X, uintptr_t s, uintptr_t ypm, uintptr_t penal,
                       double C, int l1, int max_outer, uintptr_t Z, uintptr_t Xd, uintptr_t W, uintptr_t iters,
                       uintptr_t xchg, uintptr_t err, uintptr_t stream))
HFENS_OP(lasso_cd_path, (int P, int F, int A, uintptr_t G, uintptr_t q, uintptr_t yy, uintptr_t nrows,
                         uintptr_t alphas, int max_iter, double tol, uintptr_t coefs, uintptr_t gaps,
                         uintptr_t iters, uintptr_t stream))
HFENS_OP(gram_rbf_batch, (uintptr_t Z, int F, uintptr_t probs, int P, int max_l, uintptr_t K,
                          uintptr_t stream))
HFENS_OP(smo_batch, (uintptr_t probs, int P, int max_l, uintptr_t K, uintptr_t alpha, double eps,
                     long long max_iter, uintptr_t rho, uintptr_t iters, uintptr_t gap, uintptr_t prof,
                     uintptr_t stream))
HFENS_OP(coop_resident_blocks, (uintptr_t out))
HFENS_OP(smo_coop_batch, (uintptr_t probs, int P, int W, int max_S, uintptr_t K, uintptr_t maps,
                          uintptr_t alpha, uintptr_t xchg, double eps, long long max_iter, uintptr_t rho,
                          uintptr_t iters, uintptr_t gap, uintptr_t err, uintptr_t prof, uintptr_t stream))
HFENS_OP(smo_coop_otf_batch, (uintptr_t probs, int P, int W, int F, int max_S, uintptr_t zcat, uintptr_t alpha,
                              uintptr_t xchg, double eps, long long max_iter, uintptr_t rho, uintptr_t iters,
                              uintptr_t gap, uintptr_t err, uintptr_t stream))
HFENS_OP(platt_batch,(uintptr_t probs, int P, uintptr_t part, int S, uintptr_t rowk, uintptr_t rho,
                       uintptr_t consts, uintptr_t srcmap, uintptr_t dec, uintptr_t AB, uintptr_t coop_bar,
                       uintptr_t coop_part, uintptr_t stream))
HFENS_OP(knn_mfma_item_words, (int F, uintptr_t out))
HFENS_OP(knn_mfma_prep, (uintptr_t D, uintptr_t dmask, int nd, int F, uintptr_t items, uintptr_t ny, uintptr_t stream))
HFENS_OP(knn_donors_mfma, (uintptr_t R, uintptr_t rmask, int nr, uintptr_t D, uintptr_t dmask, int nd, int F,
                           uintptr_t slot_col, uintptr_t best, uintptr_t alt, uintptr_t cnt, int s0, uintptr_t items,
                           uintptr_t ny, uintptr_t stream))
HFENS_OP(knn_donors, (uintptr_t R, uintptr_t rmask, int nr, uintptr_t D, uintptr_t dmask, int nd, int F,
                      uintptr_t slot_col, uintptr_t best, uintptr_t alt, uintptr_t cnt, int s0, uintptr_t stream))
HFENS_OP(knn_plan_host, (uintptr_t bits_, long long n, int F, int slots, uintptr_t out_, long long cap,
                         uintptr_t dims_))
HFENS_OP(knn_refine, (uintptr_t R, uintptr_t rmask, int nr, uintptr_t D, uintptr_t dmask, int nd, int F,
                      uintptr_t slot_col, uintptr_t best, uintptr_t alt, uintptr_t R64, uintptr_t D64, uintptr_t Mx,
                      uintptr_t work, long long cap, uintptr_t cnt, int s0, uintptr_t items, uintptr_t ny,
                      uintptr_t stream))
HFENS_OP(weighted_moments, (uintptr_t X, int n, int F, uintptr_t W, uintptr_t V, int P, uintptr_t Gpart,
                            uintptr_t apart, uintptr_t vpart, uintptr_t stream))
HFENS_OP(svc_oof, (uintptr_t dec, uintptr_t model, uintptr_t rho, uintptr_t AB, uintptr_t rows, uintptr_t meta,
                   int ld, int col, int n, uintptr_t stream))
HFENS_OP(svm_dec_batch, (uintptr_t zcat, uintptr_t coef, uintptr_t hcat, int F, uintptr_t probs, int P,
                         int max_h, int S, uintptr_t part, uintptr_t counts, uintptr_t stream))
HFENS_OP(svm_sv_compact, (uintptr_t zcat, uintptr_t coef, int F, uintptr_t probs, int P, uintptr_t zc, uintptr_t cc,
                          uintptr_t counts, uintptr_t stream))
HFENS_OP(libsvm_perm, (int l, long long seed, uintptr_t out_ptr))
HFENS_OP(svc_expand_host, (uintptr_t y_ptr, long long n, long long seed, uintptr_t out_ptr, uintptr_t meta_ptr))
HFENS_OP(sklearn_stump_ranks, (int T, int F, uintptr_t seeds_ptr, uintptr_t constant_ptr, uintptr_t ranks_ptr))
HFENS_OP(wsyrk_f64, (uintptr_t Phi, uintptr_t d, long long n, int r, uintptr_t part, long long part_len, uintptr_t S,
                     uintptr_t stream))
HFENS_OP(wsyrk_f32, (uintptr_t Phi, uintptr_t d, long long n, int r, uintptr_t part, long long part_len, uintptr_t S,
                     uintptr_t stream))
HFENS_OP(wsyrk_f64x, (uintptr_t Phi, uintptr_t d, long long n, int r, uintptr_t part, long long part_len, uintptr_t S,
                      uintptr_t stream))
HFENS_OP(phi_gemv, (uintptr_t Phi, uintptr_t W, long long n, int r, int k, uintptr_t Y, uintptr_t stream))
HFENS_OP(fill_dev, (uintptr_t out, long long n, uintptr_t src, uintptr_t stream))
HFENS_OP(ipm_max_step, (uintptr_t v0, uintptr_t d0, uintptr_t v1, uintptr_t d1, uintptr_t v2, uintptr_t d2,
                        uintptr_t v3, uintptr_t d3, double s0, double s1, double s2, double s3, long long n,
                        uintptr_t out, uintptr_t stream))
HFENS_OP(scale_rows_f32, (uintptr_t P, uintptr_t d, long long n, int r, uintptr_t out, uintptr_t stream))
HFENS_OP(ipm_resid, (uintptr_t c, uintptr_t a, uintptr_t y, uintptr_t P, int sp, uintptr_t b, uintptr_t nu, uintptr_t mu,
                     long long n, uintptr_t s, uintptr_t rd, uintptr_t stream))
HFENS_OP(ipm_pred, (uintptr_t a, uintptr_t s, uintptr_t nu, uintptr_t mu, uintptr_t rd, uintptr_t y, long long n,
                    uintptr_t Dinv, uintptr_t Dinv2, uintptr_t rnu, uintptr_t rmu, uintptr_t H2, uintptr_t stream))
HFENS_OP(ipm_corr, (uintptr_t a, uintptr_t s, uintptr_t nu, uintptr_t mu, uintptr_t da, uintptr_t dnu, uintptr_t dmu,
                    uintptr_t rd, uintptr_t tau, long long n, uintptr_t rnu, uintptr_t rmu, uintptr_t h, uintptr_t stream))
HFENS_OP(ipm_minv_pre, (uintptr_t Dinv, uintptr_t y, uintptr_t U, int k, long long n, uintptr_t du, uintptr_t V,
                        uintptr_t stream))
HFENS_OP(ipm_minv_post, (uintptr_t Dinv, uintptr_t y, uintptr_t du, uintptr_t P, int k, long long n, uintptr_t out,
                         uintptr_t stream))
HFENS_OP(ipm_update, (uintptr_t a, uintptr_t nu, uintptr_t mu, uintptr_t da, uintptr_t dnu, uintptr_t dmu, uintptr_t t,
                      long long n, uintptr_t a2, uintptr_t nu2, uintptr_t mu2, uintptr_t stream))
HFENS_OP(ipm_dirs, (uintptr_t Mh, int smh, uintptr_t My, int smy, uintptr_t db, uintptr_t rnu, uintptr_t rmu,
                    uintptr_t nu, uintptr_t mu, uintptr_t a, uintptr_t s, long long n, uintptr_t da, uintptr_t dnu,
                    uintptr_t dmu, uintptr_t stream))
HFENS_OP(ipm_gondzio_rhs, (uintptr_t a, uintptr_t s, uintptr_t nu, uintptr_t mu, uintptr_t da, uintptr_t dnu,
                           uintptr_t dmu, uintptr_t alpha, uintptr_t tau, long long n, uintptr_t ta, uintptr_t ts,
                           uintptr_t rhs, uintptr_t stream))
HFENS_OP(ipm_gondzio_apply, (uintptr_t Mh, int smh, uintptr_t My, int smy, uintptr_t dbc, uintptr_t da,
                             uintptr_t dnu, uintptr_t dmu, uintptr_t ta, uintptr_t ts, uintptr_t nu, uintptr_t mu,
                             uintptr_t a, uintptr_t s, long long n, uintptr_t nda, uintptr_t ndnu, uintptr_t ndmu,
                             uintptr_t stream))
HFENS_OP(ipm_select3, (uintptr_t ok, uintptr_t x0, uintptr_t x1, uintptr_t x2, long long n, uintptr_t y0,
                       uintptr_t y1, uintptr_t y2, uintptr_t stream))
HFENS_OP(phi_gemv_f32, (uintptr_t Phi, uintptr_t W, long long n, int r, int k, uintptr_t Y, uintptr_t stream))
HFENS_OP(phit_f32, (uintptr_t Phi, uintptr_t V, long long n, int r, int k, uintptr_t part, long long part_len,
                    uintptr_t out, uintptr_t stream))
HFENS_OP(scaler_batch, (uintptr_t X, long long n, int F, uintptr_t rows, uintptr_t offs, int K, long long max_rows,
                        uintptr_t part, uintptr_t mean, uintptr_t var, uintptr_t Z, uintptr_t stream))
HFENS_OP(chol_spd, (uintptr_t S, int r, uintptr_t L, uintptr_t sc, uintptr_t info, uintptr_t stream))
HFENS_OP(chol_spd_mw, (uintptr_t S, int r, uintptr_t L, uintptr_t sc, uintptr_t info, uintptr_t work, uintptr_t PT,
                       uintptr_t stream))
HFENS_OP(chol_solve, (uintptr_t L, uintptr_t sc, int r, int k, uintptr_t B, uintptr_t stream))
HFENS_OP(gbdt_stage_tick, (uintptr_t t_dev, uintptr_t stream))
HFENS_OP(gbdt_stump_stage, (int t, int B, int n, int F, int T, uintptr_t bins, long long ldb, uintptr_t nbins, int hist_len,
                            uintptr_t lo_val, uintptr_t hi_val, uintptr_t y, uintptr_t w, uintptr_t raw,
                            uintptr_t wt, uintptr_t seeds, long long row_off, double subsample, uintptr_t comm,
                            uintptr_t feat, uintptr_t blo, uintptr_t thr, uintptr_t value, uintptr_t stats,
                            uintptr_t r2, uintptr_t dev, uintptr_t bagw, uintptr_t frank, uintptr_t partials,
                            long long partials_len, double lr, double qscale, double dscale,
                            double min_leaf_q, double min_split_q, uintptr_t prof, uintptr_t t_dev,
                            int tick_in_reduce, int persist, uintptr_t bar, uintptr_t err, uintptr_t stream))
HFENS_OP(stack_infer, (uintptr_t X, int x_f64, long long n, int F, int mp, int T, int K, double ngl2e,
                       double svc_b, double probA, double probB, double gb_init, double gb_lr,
                       double lr_b, double mw0, double mw1, double mw2, double mb, uintptr_t mean,
                       uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef,
                       uintptr_t nodes, uintptr_t values, uintptr_t lr_w, uintptr_t st_off,
                       uintptr_t st_pairs, double st_base, uintptr_t out, int grid, uintptr_t stream))
HFENS_OP(stack_coalition, (uintptr_t X, long long n, uintptr_t BG, long long B, int F, int mp, int T, int K,
                           double ngl2e, double svc_b, double probA, double probB, double gb_init,
                           double gb_lr, double lr_b, double mw0, double mw1, double mw2, double mb,
                           uintptr_t mean, uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef,
                           uintptr_t nodes, uintptr_t values, uintptr_t lr_w, uintptr_t st_off,
                           uintptr_t st_pairs, double st_base, uintptr_t v, int grid, uintptr_t stream))
HFENS_OP(shapley_reduce, (uintptr_t v, long long n, int F, uintptr_t w, uintptr_t phi, uintptr_t stream))
HFENS_OP(shapley_interactions, (uintptr_t v, long long n, int F, uintptr_t u, uintptr_t phi, uintptr_t part,
                                long long part_len, uintptr_t Phi, uintptr_t stream))
HFENS_OP(stack_partial, (uintptr_t X, long long n, uintptr_t feat, uintptr_t value, long long C, int F, int mp, int T,
                         int K, double ngl2e, double svc_b, double probA, double probB, double gb_init,
                         double gb_lr, double lr_b, double mw0, double mw1, double mw2, double mb,
                         uintptr_t mean, uintptr_t inv_scale, uintptr_t svt, uintptr_t sn, uintptr_t coef,
                         uintptr_t nodes, uintptr_t values, uintptr_t lr_w, uintptr_t st_off,
                         uintptr_t st_pairs, double st_base, uintptr_t pd, uintptr_t ice, int grid,
                         uintptr_t stream))
HFENS_OP(stack_permute, (uintptr_t X, uintptr_t Xt, long long n, uintptr_t src, long long R, uintptr_t feat,
                         long long K, int F, int mp, int T, int Kn, double ngl2e, double svc_b, double probA,
                         double probB, double gb_init, double gb_lr, double lr_b, double mw0, double mw1,
                         double mw2, double mb, uintptr_t mean, uintptr_t inv_scale, uintptr_t svt, uintptr_t sn,
                         uintptr_t coef, uintptr_t nodes, uintptr_t values, uintptr_t lr_w, uintptr_t st_off,
                         uintptr_t st_pairs, double st_base, uintptr_t S, int grid, uintptr_t stream))
HFENS_OP(rank_lds_rows, (uintptr_t out))
HFENS_OP(rank_rows, (uintptr_t S, uintptr_t y, uintptr_t ss, uintptr_t ys, long long n, long long M, int use_lds,
                     uintptr_t ws, long long ws_slices, uintptr_t a2, uintptr_t auroc, uintptr_t ap,
                     uintptr_t brier, int grid, uintptr_t stream))
HFENS_OP(ws_init, (uintptr_t probs, int P, int max_l, uintptr_t zcat, int F, uintptr_t zn, uintptr_t alpha,
                   uintptr_t G, uintptr_t states, uintptr_t keys, long long n, uintptr_t hist, uintptr_t gkey,
                   uintptr_t stream))
HFENS_OP(cascade_where, (uintptr_t tab, int Q, long long max_len, uintptr_t where, uintptr_t stream))
HFENS_OP(ws_seed, (uintptr_t probs, int P, int max_l, uintptr_t zcat, int F, uintptr_t zn, uintptr_t aseed,
                   uintptr_t alpha, uintptr_t G, uintptr_t keys, long long n, uintptr_t gkey, uintptr_t stream))
HFENS_OP(ws_steps, (uintptr_t probs, int P, int max_l, uintptr_t zcat, int F, uintptr_t zn, uintptr_t alpha,
                    uintptr_t G, uintptr_t states, uintptr_t wsz, uintptr_t wsn, uintptr_t wdc, uintptr_t wsprev,
                    uintptr_t wsidx, uintptr_t keys, long long n, uintptr_t gkey, double eps, int max_outer, int max_inner,
                    double inner_frac, int n_iter, uintptr_t prof, int inner_threads, int q, uintptr_t stream))
HFENS_OP(ws_steps_kc, (uintptr_t probs, int P, int max_l, uintptr_t zcat, int F, uintptr_t zn, uintptr_t alpha,
                       uintptr_t G, uintptr_t states, uintptr_t wsz, uintptr_t wsn, uintptr_t wdc, uintptr_t wsprev,
                       uintptr_t keys, long long n, uintptr_t gkey, uintptr_t cand, double eps, int max_outer,
                       int max_inner, double inner_frac, int n_iter, uintptr_t prof, uintptr_t stream))
HFENS_OP(ws_kc_cand_len, (long long max_l, uintptr_t out))
HFENS_OP(ws_finalize, (uintptr_t probs, int P, uintptr_t states, uintptr_t alpha, uintptr_t G, uintptr_t rho,
                       uintptr_t iters, uintptr_t inner, uintptr_t gap, uintptr_t stream))
HFENS_OP(binned_stump_raw, (uintptr_t bins, long long n, int F, uintptr_t tables, int B, uintptr_t init,
                            uintptr_t out, uintptr_t stream))
HFENS_OP(forest_fp8, (uintptr_t bins, long long ldb, long long n, int F, int T, int d, uintptr_t nodes, uintptr_t bfrag,
                      int Q, int S, uintptr_t inv_scale, uintptr_t init, uintptr_t out, uintptr_t stream))
HFENS_OP(quantize_bins, (uintptr_t X, int f64, long long n, int F, uintptr_t edges, int K, uintptr_t nbins,
                         uintptr_t out, long long ldb, uintptr_t stream))
HFENS_OP(stack_predict_host, (int n, int F, uintptr_t X_, uintptr_t mean_, uintptr_t scale_, int nsv, uintptr_t sv_,
                              uintptr_t coef_, double gamma, double svc_icpt, double probA, double probB, int T,
                              int K, uintptr_t feat_, uintptr_t thr_, uintptr_t left_, uintptr_t right_,
                              uintptr_t value_, double gbc_init, double lr, uintptr_t lrc_, double lr_icpt,
                              uintptr_t meta_, double meta_icpt, uintptr_t out_))
HFENS_OP(wsyrk_part_len, (long long n, int r, uintptr_t out))
HFENS_OP(phit_part_len, (long long n, int r, int k, uintptr_t out))
HFENS_OP(gbdt_stage_plan, (long long n, int B, int hist_len, int ncu, uintptr_t out))
HFENS_OP(xgmi_alloc, (long long bytes, int uncached, uintptr_t out))
HFENS_OP(xgmi_free, (uintptr_t p))
HFENS_OP(xgmi_ipc_handle, (uintptr_t p, uintptr_t out))
HFENS_OP(xgmi_ipc_open, (uintptr_t handle, uintptr_t out))
HFENS_OP(xgmi_ipc_close, (uintptr_t p))
HFENS_OP(xgmi_allreduce, (uintptr_t local, long long count, int dtype, int op, uintptr_t peers, int W, int me,
                          int k, long long cap, long long epoch_base, int t_host, uintptr_t t_dev, uintptr_t err,
                          double timeout_s, uintptr_t stream))
HFENS_OP(xgmi_allreduce_i64, (uintptr_t local, long long count, uintptr_t peers, int W, int me, int k, long long cap,
                              long long epoch_base, int t_host, uintptr_t t_dev, uintptr_t err, double timeout_s,
                              uintptr_t stream))
HFENS_OP(gbdt_ranks_dev, (int T, int B, int F, int n, uintptr_t bins, long long ldb, uintptr_t w, uintptr_t seeds,
                          uintptr_t ranks, uintptr_t stream))
HFENS_OP(oof_trees, (uintptr_t X, int F, uintptr_t rows, uintptr_t model, long long m, int T, int B, int NN,
                     uintptr_t feat, uintptr_t thr, uintptr_t value, uintptr_t init, double lr, uintptr_t meta, int ld,
                     int col, uintptr_t stream))
HFENS_OP(oof_linear, (uintptr_t X, int F, uintptr_t rows, uintptr_t model, long long m, uintptr_t W, int F1,
                      int has_icpt, double icpt_scale, uintptr_t meta, int ld, int col, uintptr_t stream))
HFENS_OP(svm_gamma, (uintptr_t Z, uintptr_t offs, int K, int F, uintptr_t gamma, uintptr_t ngl2e, uintptr_t stream))
HFENS_OP(svm_patch_f32, (uintptr_t base, int stride, int off, int count, uintptr_t fit_of, uintptr_t src,
                         uintptr_t stream))
HFENS_OP(knn_plan_dev, (uintptr_t X, long long n, int F, uintptr_t centre, uintptr_t dmax, uintptr_t rows,
                        uintptr_t rbits, uintptr_t slot, int G, uintptr_t R32, uintptr_t R64, uintptr_t colmax,
                        uintptr_t Mx, uintptr_t cnt, uintptr_t bcnt, uintptr_t stream))
HFENS_OP(knn_apply, (uintptr_t X, long long n, int F, uintptr_t rows, uintptr_t slot, uintptr_t best, uintptr_t fitX,
                     uintptr_t colmean, uintptr_t cnt, uintptr_t stream))
HFENS_OP(host_store, (uintptr_t src, uintptr_t dst_host, long long n, int elem_bytes, uintptr_t stream))
HFENS_OP(rbf_f64, (uintptr_t Z, long long l, uintptr_t L, int m, int F, double gamma, uintptr_t out, uintptr_t stream))
HFENS_OP(bootstrap_lds_rows, (uintptr_t out))
HFENS_OP(bootstrap_metrics, (uintptr_t y, uintptr_t gfirst, uintptr_t glast, uintptr_t map, long long n, long long p0,
                             long long k0, int G, long long seed, long long b0, long long nb, int use_lds,
                             uintptr_t ws, long long ws_slices, uintptr_t auroc, uintptr_t ap, uintptr_t a2,
                             uintptr_t pn, uintptr_t conf, uintptr_t tpr, int grid, uintptr_t stream))
HFENS_OP(calibration_lds_rows, (uintptr_t out))
HFENS_OP(bootstrap_calibration, (uintptr_t y, uintptr_t map, uintptr_t p, uintptr_t l, uintptr_t bin_end, uintptr_t thr,
                                 long long n, long long p0, int K, int T, long long seed, long long b0, long long nb,
                                 int use_lds, uintptr_t ws, long long ws_slices, uintptr_t pn, uintptr_t brier,
                                 uintptr_t sum_p, uintptr_t bin_n, uintptr_t bin_pos, uintptr_t bin_sum_p, uintptr_t dc,
                                 uintptr_t status, uintptr_t coef, uintptr_t iters, int grid, uintptr_t stream))
HFENS_OP(compare_lds_rows, (uintptr_t out))
HFENS_OP(bootstrap_compare, (uintptr_t y, uintptr_t rowmap, uintptr_t order, uintptr_t ys, uintptr_t gfirst,
                             uintptr_t glast, uintptr_t k0, uintptr_t hi, uintptr_t p, long long n, long long p0, int M,
                             long long seed, long long b0, long long nb, int use_lds, uintptr_t ws,
                             long long ws_slices, uintptr_t auroc, uintptr_t ap, uintptr_t a2, uintptr_t pn,
                             uintptr_t conf, uintptr_t reclass, uintptr_t sums, int grid, uintptr_t stream))
#undef HFENS_OP
