// The engine options (include/stts2.h STTS_OPT_*, where each key's meaning is documented): one row per live key.
// Adding or pruning an option is one row here, its #define + comment in the header and its row in engine.py's _OPTS.
// From this list come the globals' definitions, stts_set_option and stts_get_option (options.cpp) and the extern
// declarations below; the engines read the plain ints.  Retired keys (3, 9, 26, 28) have no row: STTS_EINVAL.
#pragma once

// What stts_set_option does with a value:
//   OPT_BOOL   stores value != 0
//   OPT_RAW    stores the value as it is (bit masks and mode numbers the engines interpret)
//   OPT_RANGE  stores a value in [lo, hi], and `fallback` for any other
//   OPT_MIN0   stores a value >= 0 and refuses a negative one with STTS_EINVAL
enum { OPT_BOOL, OPT_RAW, OPT_RANGE, OPT_MIN0 };

// X(key, variable, production default, rule, lo, hi, fallback)      (lo, hi, fallback: OPT_RANGE rows only)
#define STTS_OPTIONS(X)                                                                                              \
  X(STTS_OPT_RESCONV, g_opt_resconv, 1, OPT_BOOL, 0, 0, 0)         /* conv1d.hip st_conv1d routing */                \
  X(STTS_OPT_GRID_CAP, g_opt_grid_cap, 0, OPT_RANGE, 0, INT_MAX, 0) /* every persistent launcher; negative = off */  \
  X(STTS_OPT_DEBUG, g_opt_debug, 0, OPT_RAW, 0, 0, 0)              /* ConvParams::dbg (timing experiments only) */    \
  X(STTS_OPT_STATS_SLOTS, g_opt_stats_slots, 0, OPT_RANGE, 0, INT_MAX, 0) /* plan.cpp with_ctx; 0 = automatic */      \
  X(STTS_OPT_SMALL_TILES, g_opt_small_tiles, 1, OPT_BOOL, 0, 0, 0) /* conv1d.hip */                                  \
  X(STTS_OPT_BIGCONV, g_opt_bigconv, 2, OPT_RANGE, 1, 5, 2)        /* bigconv.hip / bigconv2.hip */                  \
  X(STTS_OPT_HEAD, g_opt_head, 1, OPT_BOOL, 0, 0, 0)               /* conv1d.hip -> head.hip */                      \
  X(STTS_OPT_FRONT, g_opt_front, 1, OPT_RANGE, 0, 2, 1)            /* bigconv2.hip st_front_eligible */              \
  X(STTS_OPT_PW, g_opt_pw, 1, OPT_RANGE, 0, 2, 1)                  /* pwgemm.hip */                                  \
  X(STTS_OPT_SPLITK, g_opt_splitk, 1, OPT_BOOL, 0, 0, 0)           /* pwgemm.hip st_pw_split_eligible */             \
  X(STTS_OPT_EXP, g_opt_exp, 0, OPT_RAW, 0, 0, 0)                  /* bits 32 / 64 bigconv2.hip, 32768 resconv.hip */ \
  X(STTS_OPT_UPS, g_opt_ups, 1, OPT_RANGE, 0, 2, 1)                /* bigconv2.hip st_ups_eligible */                \
  X(STTS_OPT_WGRAD, g_opt_wgw, 1, OPT_BOOL, 0, 0, 0)               /* convbwd.hip k_wgrad_bf16w */                   \
  X(STTS_OPT_PLAINRC, g_opt_plainrc, 1, OPT_BOOL, 0, 0, 0)         /* resconv.hip */                                 \
  X(STTS_OPT_MSDFOLD, g_opt_msdfold, 1, OPT_BOOL, 0, 0, 0)         /* plan.cpp build_msd: read at model creation */  \
  /* RCPP's fallback is 1, NOT its default 3: 1 was the default when the rule was written, and an out-of-range  */   \
  /* value has selected mode 1 ever since.  Kept as it is; aligning the two is a behaviour change. */                \
  X(STTS_OPT_RCPP, g_opt_rcpp, 3, OPT_RANGE, 0, 3, 1)              /* resconv.hip */                                 \
  X(STTS_OPT_RESSPLIT, g_opt_ressplit, 1, OPT_BOOL, 0, 0, 0)       /* ressplit.hip */                                \
  X(STTS_OPT_BF16F, g_opt_bf16f, 0, OPT_BOOL, 0, 0, 0)             /* convbwd.hip */                                 \
  X(STTS_OPT_YF32, g_opt_yf32, 1, OPT_BOOL, 0, 0, 0)               /* convbwd.hip */                                 \
  X(STTS_OPT_COUT1, g_opt_cout1, 1, OPT_BOOL, 0, 0, 0)             /* convbwd.hip k_conv_cout1 */                    \
  X(STTS_OPT_BRANCHES, g_opt_branches, 8, OPT_MIN0, 0, 0, 0)       /* plan.cpp decoder_forward */                    \
  X(STTS_OPT_NBRANCH, g_opt_nbranch, 64, OPT_MIN0, 0, 0, 0)        /* plan.cpp decoder_forward */                    \
  X(STTS_OPT_BIGSPLIT, g_opt_bigsplit, 1, OPT_RAW, 0, 0, 0)        /* bigconv2.hip st_bigsplit_eligible */           \
  /* BIG64 5: SP on 4-wave blocks is 2-7 % faster per launch than on 8-wave (profiles/r05_ab_big64.txt) */           \
  X(STTS_OPT_BIG64, g_opt_big64, 5, OPT_RAW, 0, 0, 0)              /* bigconv2.hip st_big64_eligible */              \
  X(STTS_OPT_SEGPART, g_opt_segpart, 1, OPT_RAW, 0, 0, 0)          /* conv1d.hip st_seg_choice */                    \
  X(STTS_OPT_RCOCC, g_opt_rcocc, 1, OPT_RAW, 0, 0, 0)              /* resconv.hip */

#define STTS_OPT_EXTERN(key, var, def, rule, lo, hi, fallback) extern int var;
STTS_OPTIONS(STTS_OPT_EXTERN)
#undef STTS_OPT_EXTERN
