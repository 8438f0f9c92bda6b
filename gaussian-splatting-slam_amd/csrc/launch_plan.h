// launch_plan.h - which kernel form a frame gets: the native switches of the environment, read in ONE place, and the pure functions
// that turn them and a frame's sizes into a launch plan.  Host only, plain C++17, no HIP header: tests/test_launch_plan_cpu.py
// compiles it into a stand-alone program and holds every plan to the record of the launchers this header replaced.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// ---- the size thresholds ---------------------------------------------------------------------------------------------------------
// One wave per tile needs enough tiles to keep 1024 SIMDs busy: below ~6 tiles per SIMD (720p: 3600 tiles) the four-waves-per-tile
// form (same results up to summation order inside a tile) has the shorter critical path.
constexpr int GSR_PLAN_QUAD_BELOW_TILES = 6000;
// The walk order pays where a launch runs in several rounds of resident workgroups; a grid that is resident at once - 256 CUs x 5
// four-wave workgroups - has no late starters to reorder: 256 tiles 0.054 -> 0.056 ms with it, 3600 tiles 0.166 -> 0.150 ...
constexpr int GSR_PLAN_WALK_ABOVE_TILES = 1280;
// ... nor does a launch of many rounds gain what its record gathers lose in locality (4K, 32 400 tiles = 6.3 rounds of one-wave
// workgroups: 1.381 -> 1.407 ms with the walk order)
constexpr int GSR_PLAN_WALK_UPTO_TILES = 24000;
// the colour pass goes to a side stream, beside the sorts, from this many Gaussians
constexpr int GSR_PLAN_ASIDE_FROM_P = 200000;
// SSIM forward, two tiles per workgroup: the pipeline pays once the launch runs in several rounds of resident workgroups
constexpr long long GSR_PLAN_SSIM_PAIR_FROM_WG = 4096;
// the emission kernel's LDS histograms cover two radix passes = 16 tile bits: a frame of more than 65536 tiles takes the chain
constexpr int GSR_PLAN_FUSED_BINS_MAX_BITS = 16;
// frames with at least this many instances flag their gradient records (gsr_common.h, gsr_flags_on)
#ifndef GSR_FLAGS_MIN_R
#define GSR_FLAGS_MIN_R 2500000u
#endif

// ---- the switches ----------------------------------------------------------------------------------------------------------------
// One field per native switch, holding what its parse keeps.  An entry point reads the scopes it needs once per call - the tests
// change the per-call switches inside one process - and hands the record down; a field outside the scopes read keeps its default.
enum GsrSwitchScope : unsigned {
  GSR_SW_BACKWARD = 1u << 0,         // bwd_*
  GSR_SW_RENDER = 1u << 1,           // fwd_mask, cull_*, tile_hist
  GSR_SW_ASYNC = 1u << 2,            // shade_stream
  GSR_SW_SORT = 1u << 3,             // force_lookback_timeout
  // read once per process, each where it is first needed:
  GSR_SW_TRACE = 1u << 4,
  GSR_SW_COUNT_TIMEOUT = 1u << 5,
  GSR_SW_SSIM = 1u << 6,
  GSR_SW_FLAGS_MIN_R = 1u << 7,
  GSR_SW_ALL = 0xFFu,
};

struct GsrSwitches {
  // GSR_BWD_FORM=quad|tile forces a compositing backward form: "quad" the four-wave one, any other value the one-wave one
  enum Form { FORM_BY_SIZE, FORM_QUAD, FORM_TILE } bwd_form = FORM_BY_SIZE;
  // GSR_BWD_MASK=0: the one-wave form without its hit masks
  bool bwd_mask = true;
  // GSR_BWD_LPT=0: tiles in index order (the A/B of the walk classes, profiles/r04_bwd_lpt_ab.txt); =1 forces the walk order for
  // any grid.  -1: neither
  int bwd_lpt = -1;
  // issue priority for long walks: thresholds from the frame itself (-1, the default), GSR_BWD_PRIO="t1,t2,t3" fixes them, "0" =
  // none (anything but three integers: -2)
  int bwd_prio[3] = {-1, -1, -1};
  // GSR_BWD_REDUCE=mfma (opt-in, measured SLOWER: 0.52 against 0.42 ms at C3, profiles/r04_bwd_mx_ab.txt) takes the sums with
  // v_mfma_f32_16x16x4_f32 (k_render_bwd_tile_mx); the default is the v_permlane / DPP halving tree
  bool bwd_reduce_mfma = false;
  // GSR_FWD_MASK=1 selects the masked walk (measured: 0.208 against 0.179 ms at C3, profiles/r04_fwd_mask_ab.txt - not the default)
  bool fwd_mask = false;
  // GSR_CULL_MARGIN="q8,add": cut-off margin of the depth-truncated lists: 1.75 x the entries a tile needed + 48 (measured,
  // profiles/r04_tile_cull.txt: 1.25 x + 16 flags 54 % of the frames of a run that trains from scratch, 1.5 x + 32 1 %,
  // 1.75 x + 48 none; C3 and the 2 x splats scene)
  unsigned cull_mq8 = 448, cull_madd = 48;
  // GSR_SHADE_STREAM=0|1: the colour pass on the caller's stream | on a side stream; negative (unset): by the number of Gaussians
  int shade_stream = -1;
  // GSR_TILE_HIST=0: the round-3 binning chain (k_radix_hist_all, k_finalize_bins) instead of the fused one, for the A/B
  bool tile_hist = true;
  // GSR_TEST_FORCE_LOOKBACK_TIMEOUT=1: the last radix pass behaves as if a look-back wait had timed out (tests)
  bool force_lookback_timeout = false;
  // GSR_TRACE (set at all): name every stage on stderr as it completes
  bool trace = false;
  // GSR_COUNT_TIMEOUT_S: how long a caller waits for num_rendered before it gives up
  double count_timeout_s = 120.0;
  // GSR_SSIM_TPW > 0: tiles per workgroup of the SSIM forward (profiles/README.md: 2 ... 8 measured, 2 stays)
  int ssim_tpw = 0;
  // GSR_FLAGS_MIN_R: the START value of the flags threshold (0 = always: how the seeded sweeps run their small scenes through the
  // flagged form); gsr_debug_set_flags_min_r changes the live one
  unsigned flags_min_r = GSR_FLAGS_MIN_R;
};

// The only place that names a switch.  `get`: the lookup (the library passes the C library's, a test one into its own table).
template <class Lookup>      // const char* get(const char* name), nullptr for a name that is not set
inline GsrSwitches gsr_switches_read(Lookup get, unsigned scopes = GSR_SW_ALL) {
  GsrSwitches sw;
  const char* v;
  if (scopes & GSR_SW_BACKWARD) {
    if ((v = get("GSR_BWD_FORM"))) sw.bwd_form = !strcmp(v, "quad") ? GsrSwitches::FORM_QUAD : GsrSwitches::FORM_TILE;
    if ((v = get("GSR_BWD_MASK"))) sw.bwd_mask = strcmp(v, "0") != 0;
    if ((v = get("GSR_BWD_LPT"))) sw.bwd_lpt = v[0] == '0' ? 0 : (v[0] == '1' ? 1 : -1);
    if ((v = get("GSR_BWD_PRIO"))) {
      int* p = sw.bwd_prio;
      if (sscanf(v, "%d,%d,%d", &p[0], &p[1], &p[2]) != 3) p[0] = p[1] = p[2] = -2;
    }
    if ((v = get("GSR_BWD_REDUCE"))) sw.bwd_reduce_mfma = !strcmp(v, "mfma");
  }
  if (scopes & GSR_SW_RENDER) {
    if ((v = get("GSR_FWD_MASK"))) sw.fwd_mask = !strcmp(v, "1");
    if ((v = get("GSR_CULL_MARGIN"))) sscanf(v, "%u,%u", &sw.cull_mq8, &sw.cull_madd);
    if ((v = get("GSR_TILE_HIST"))) sw.tile_hist = v[0] != '0';
  }
  if ((scopes & GSR_SW_ASYNC) && (v = get("GSR_SHADE_STREAM"))) sw.shade_stream = atoi(v);
  if ((scopes & GSR_SW_SORT) && (v = get("GSR_TEST_FORCE_LOOKBACK_TIMEOUT"))) sw.force_lookback_timeout = v[0] == '1';
  if (scopes & GSR_SW_TRACE) sw.trace = get("GSR_TRACE") != nullptr;
  if ((scopes & GSR_SW_COUNT_TIMEOUT) && (v = get("GSR_COUNT_TIMEOUT_S"))) sw.count_timeout_s = atof(v);
  if ((scopes & GSR_SW_SSIM) && (v = get("GSR_SSIM_TPW"))) sw.ssim_tpw = atoi(v);
  if ((scopes & GSR_SW_FLAGS_MIN_R) && (v = get("GSR_FLAGS_MIN_R")) && *v) sw.flags_min_r = (unsigned)strtoul(v, nullptr, 10);
  return sw;
}

// ---- the plans: no globals, no HIP, no I/O ---------------------------------------------------------------------------------------
// compositing forward: k_render_fwd<false, masked, alpha, touch>
struct GsrRenderFwdPlan {
  bool masked, alpha, touch;     // touch: n_touched (gsr_render_extras), the TOUCH instantiations; alpha: out_alpha, likewise
  unsigned mq8, madd;            // the cut-off margin
};
inline GsrRenderFwdPlan gsr_plan_render_fwd(const GsrSwitches& sw, bool has_alpha, bool has_touch) {
  return {sw.fwd_mask, has_alpha, has_touch, sw.cull_mq8, sw.cull_madd};
}
inline void gsr_plan_describe(const GsrRenderFwdPlan& p, char* out, size_t n) {
  snprintf(out, n, "k_render_fwd<M=%d,A=%d,C=%d> margin=%u,%u", p.masked, p.alpha, p.touch, p.mq8, p.madd);
}

// compositing backward: k_render_bwd<depth, alpha> (four waves per tile), k_render_bwd_tile<depth, mask, alpha> (one wave) or
// k_render_bwd_tile_mx<depth, alpha> (one wave, sums on the matrix pipe: always masked, never in walk order)
struct GsrRenderBwdPlan {
  enum Form { QUAD, TILE, TILE_MX } form;
  bool depth, mask, alpha;       // alpha: dL_dalpha (gsr_render_extras), the ALPHA instantiations; mask: the one-wave form's only
  bool walk;                     // tiles longest walk first (the classes the forward filed them under), not in index order (not mx)
  int prio[3];                   // (the one-wave forms)
  unsigned flags_min_r;          // the projection backward of the same step gets the same value
};
inline GsrRenderBwdPlan gsr_plan_render_bwd(const GsrSwitches& sw, int tiles, bool has_depth, bool has_alpha, unsigned flags_min_r) {
  GsrRenderBwdPlan p;
  const bool quad = sw.bwd_form == GsrSwitches::FORM_BY_SIZE ? tiles < GSR_PLAN_QUAD_BELOW_TILES : sw.bwd_form == GsrSwitches::FORM_QUAD;
  const bool mx = !quad && sw.bwd_mask && sw.bwd_reduce_mfma;
  p.form = quad ? GsrRenderBwdPlan::QUAD : (mx ? GsrRenderBwdPlan::TILE_MX : GsrRenderBwdPlan::TILE);
  p.depth = has_depth;
  p.mask = sw.bwd_mask;
  p.alpha = has_alpha;
  const bool by_size = tiles > GSR_PLAN_WALK_ABOVE_TILES && tiles <= GSR_PLAN_WALK_UPTO_TILES;
  p.walk = sw.bwd_lpt != 0 && (by_size || sw.bwd_lpt == 1);
  for (int i = 0; i < 3; i++) p.prio[i] = sw.bwd_prio[i];
  p.flags_min_r = flags_min_r;
  return p;
}
inline void gsr_plan_describe(const GsrRenderBwdPlan& p, char* out, size_t n) {
  if (p.form == GsrRenderBwdPlan::QUAD)
    snprintf(out, n, "k_render_bwd<D=%d,A=%d> walk=%d flags_min_r=%u", p.depth, p.alpha, p.walk, p.flags_min_r);
  else if (p.form == GsrRenderBwdPlan::TILE)
    snprintf(out, n, "k_render_bwd_tile<D=%d,M=%d,A=%d> walk=%d prio=%d,%d,%d flags_min_r=%u", p.depth, p.mask, p.alpha, p.walk,
             p.prio[0], p.prio[1], p.prio[2], p.flags_min_r);
  else
    snprintf(out, n, "k_render_bwd_tile_mx<D=%d,A=%d> prio=%d,%d,%d flags_min_r=%u", p.depth, p.alpha, p.prio[0], p.prio[1],
             p.prio[2], p.flags_min_r);
}

// whether the colour pass of a non-blocking forward runs on the side stream, beside the sorts (late: the caller deferred it behind
// an event; precomp: colours given; has_sh: there are coefficients to evaluate; debug: every stage is waited for)
inline bool gsr_plan_shade_aside(const GsrSwitches& sw, int P, bool late, bool precomp, bool has_sh, bool debug) {
  const bool want = sw.shade_stream < 0 ? P >= GSR_PLAN_ASIDE_FROM_P : sw.shade_stream != 0;
  return want && !late && !precomp && has_sh && !debug;
}

// tile-local binning: the emission counts the tile sort's digit histograms and the sort's last pass leaves the tile ranges
inline bool gsr_plan_fused_bins(const GsrSwitches& sw, bool tile_local, int tile_bits) {
  return tile_local && sw.tile_hist && tile_bits <= GSR_PLAN_FUSED_BINS_MAX_BITS;
}

// tiles per workgroup of the SSIM forward on a gx x gy x planes grid of tiles
inline int gsr_plan_ssim_tpw(const GsrSwitches& sw, int gx, int gy, int planes) {
  if (sw.ssim_tpw > 0) return sw.ssim_tpw;
  return (long long)gx * gy * planes >= GSR_PLAN_SSIM_PAIR_FROM_WG ? 2 : 1;
}
