"""The column order of srmi_gradient's fp64 outputs (include/srmi.h, "the gradient score"): one
copy for srmi.gradient, srmi.results and the oracle.  No torch, no library."""
GRADIENT_SUMS = ("sum_mag_pred", "sum_mag_truth", "sum_dmag2", "sum_dvec2", "sum_dot", "sum_pred2", "sum_truth2")
GRADIENT_STATS = ("mean_pred", "mean_truth", "sharpness", "rmse_mag", "rmse_vec", "cosine")
