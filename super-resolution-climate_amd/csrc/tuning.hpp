// The compile-time knobs of the srmi kernels, in one place: every value of each is live
// code or a plain number, and the values below are the production build.  The kernel forms
// that lost their A/Bs (DESIGN.md sections 3-4, profiles/) are not selectable here: their
// code was removed and builds from the history.  Run-time choices (tests' reference
// engines) are the srmi_model_config.flags bits, include/srmi.h.
#pragma once

// Write-through (sc1) stores for the large outputs (common.hpp st_wt*): the kernel
// boundary then finds no dirty lines to flush (the slabs alone: +1.1 % in the step).
#ifndef SRMI_TRAIN_WT
#define SRMI_TRAIN_WT 1
#endif
// the one-launch inference RCAB (rcab_infer.hip): write-back stores -- t is re-read by
// the workgroup that wrote it and the pair by the next launch (+1 % C5 over write-through)
#ifndef SRMI_INFER_WT
#define SRMI_INFER_WT 0
#endif

// rcab_infer.hip defines SRMI_TU_INFER before its includes: the inference policies (the
// stores here; the deferred conv epilogues, conv64_body.hpp conv64_defers)
#ifdef SRMI_TU_INFER
#define SRMI_WT SRMI_INFER_WT
#else
#define SRMI_WT SRMI_TRAIN_WT
#endif

// waves per workgroup of the exact-fp32 conv (conv_f32.hip)
#ifndef SRMI_F32_NW
#define SRMI_F32_NW 8
#endif

// workgroups of the tail conv's forward (small.hip tail_fwd_launch)
#ifndef SRMI_TAIL_FWD_BLOCKS
#define SRMI_TAIL_FWD_BLOCKS 512
#endif

// 8-channel groups per thread of the CA elementwise passes (small.hip): 4 amortises the
// per-block MLP over twice the data of 2 (ca_fwd 22.6 -> 20.0 us, ca_bwd 15.1 -> 13.7 us)
#ifndef SRMI_CA_VEC
#define SRMI_CA_VEC 4
#endif

// SRMI_STAMPS (undefined in production): s_memtime stamps per workgroup phase into
// ConvParams / WgradParams .stamps (srmi_debug_conv_stamps, tools/stamps_run.sh)
