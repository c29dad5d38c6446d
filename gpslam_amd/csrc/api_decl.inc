// api_decl.inc -- the entry points of a precision namespace (api_impl.inc, api_iterate.inc), included inside namespace impl64 / impl32 by
// every translation unit that calls across them
int gpslam_hip_block_tridiag_solve(gpslam_hip_handle *h, int32_t N, const double *D, const double *O,
                                   const double *g, double *x);
int gpslam_hip_compile(gpslam_hip_handle *h);
int gpslam_hip_error(gpslam_hip_handle *h, double *err);
int gpslam_hip_fs_interface(gpslam_hip_handle *h, void **send, size_t *send_bytes, void **recv, size_t *recv_bytes);
int gpslam_hip_fs_lm_trial_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_fs_lm_trial_phase2(gpslam_hip_handle *h, double *out6);
int gpslam_hip_fs_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_fs_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_get_between_pairs_weights(gpslam_hip_handle *h, double *w);
int gpslam_hip_get_meas_weights(gpslam_hip_handle *h, int32_t kind, double *w);
int gpslam_hip_get_rows(gpslam_hip_handle *h, int32_t *n_rows, double *rowLR, double *rowE, double *rowM, int32_t *rowLm);
int gpslam_hip_interface_recv(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
int gpslam_hip_interface_send(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
int gpslam_hip_iterate_gn(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_iterate_lm(gpslam_hip_handle *h, double *lambda, const gpslam_hip_params *p, gpslam_hip_stats *st);
int gpslam_hip_iterate_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_iterate_phase2(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_iterate_phase2a(gpslam_hip_handle *h);
int gpslam_hip_iterate_phase2b(gpslam_hip_handle *h, gpslam_hip_stats *st);
int gpslam_hip_landmark_reduce_buffer(gpslam_hip_handle *h, void **dev_ptr, size_t *bytes);
int gpslam_hip_linearize_gp(gpslam_hip_handle *h, double *errors, double *jacobians);
int gpslam_hip_linearize_meas(gpslam_hip_handle *h, int32_t kind, double *errors, double *jacobians);
int gpslam_hip_lm_begin(gpslam_hip_handle *h);
int gpslam_hip_lm_reject(gpslam_hip_handle *h);
int gpslam_hip_lm_trial_phase1(gpslam_hip_handle *h, double lambda);
int gpslam_hip_lm_trial_phase2(gpslam_hip_handle *h, double *out6);
int gpslam_hip_normal_equations(gpslam_hip_handle *h, double *D, double *O, double *g, double *B);
int gpslam_hip_optimize(gpslam_hip_handle *h, const gpslam_hip_params *p, gpslam_hip_stats *st);
int gpslam_hip_run_gn(gpslam_hip_handle *h, int32_t iters, gpslam_hip_stats *st, double *out5);
int gpslam_hip_time_kernel(gpslam_hip_handle *h, int32_t which, int32_t reps, double *avg_ms);
// The launchers (api_impl.inc) a feature's translation unit may call; what each does stands at its definition, the default arguments here.
int launch_factors(gpslam_hip_handle *h, const LaunchMode &m, int pass, int slot, bool e32 = false);
int launch_assemble(gpslam_hip_handle *h, const LaunchMode &m, bool save_g, int pass = 0);
int launch_solve(gpslam_hip_handle *h, const LaunchMode &m, double lambda);
int launch_retract(gpslam_hip_handle *h, const LaunchMode &m, int slot);
int launch_meas_inspect(gpslam_hip_handle *h, int kind, int first, int count, void *out_e, void *out_J);
