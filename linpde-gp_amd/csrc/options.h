// The tuning options of a context (lpgp_ctx derives from lpgp::Options), one row each in the table of options.cpp, which
// lpgp_init (environment), lpgp_get_option and lpgp_set_option walk.  Plain C++: also in the `build.sh --host-asan` library.
#pragma once

#include <cstdint>

namespace lpgp {

struct Options {
  int reserve_cus = 32;                // CUs the masked update streams (s_upd, s_outer) leave to the panel chain (0: no mask; read at init)
  int reserve_narrow = 64;             // ... and s_upd_narrow, once the chain bounds the pipeline (read at init)
  int single_stream = 0;               // LPGP_SINGLE_STREAM: all streams of the context alias s_main (ranks sharing one GPU in tests; read at init)
  int64_t nb_outer = 2048;             // far columns are updated once per nb_outer columns (0 or <= nb: every panel) ...
  int nb_outer_min_tiles = 192;        // ... while more than this many tile columns remain
  // ride-along substitution (potrf_predict_blocked) ...
  int ride_stream = 1 + 8 * 7;         // ... runs on (first + 8 * second stream; potrf.hip): 0 s_outer, 1 s_upd_all, 2 s_upd_narrow, 3 the panel stream, 4 s_upd, 7 none
  int ride_old_ungated = 1;            // ... the steps of old panels (block append) are not held back by the gate
  int ride_occ3 = 1;                   // ... its updates may use the three-workgroups-per-CU kernel
  int append_split = 0;                // (OFF: measured flat, c3 50.3-50.8 either way, profiles/r06_append_split_ab.txt) block append: the last old panel's update of the new block split into the first new panel's columns (panel stream) and the
  int append_split_min_tiles = 16;     // remainder (update stream, under the first new chain), for new blocks of at least this many tile rows (LPGP_APPEND_SPLIT)
  int ride_b_on_ride = 0;              // ... the factorisation's remainder updates queue on the substitution's stream once its gate is open (LPGP_RIDE_B_ON_RIDE)
  int ride_aug = 0;                    // ... or, where the matrix has room for it, as ROWS of the matrix being factored (potrf.hip: augmented form; LPGP_RIDE_AUG)
  // resident panel chain (chain.hip): panels of four tiles with at most this many tile rows below them run their whole chain in
  // ONE launch whose workgroups hand over through device flags (-1: never)
  int chain_resident_max_rows = 32;
  int chain_ahead = 1;                 // resident chain: the look-ahead update by the previous panel rides in front of the NEXT panel's chain (one launch per panel
                                       // where two chains follow each other; LPGP_CHAIN_AHEAD=0: a launch of its own, round 5)
  int chain_ahead_min_rows = 12;       // ... where at least this many tile rows lie below that panel (LPGP_CHAIN_AHEAD_MIN_ROWS)
  int chain_resident2_max_rows = 0;    // ... and panels with MORE rows below (up to this many tile rows) as TWO launches that talk through the same flags: factor + in-block
                                       // workgroups on the panel stream, the rows below -- 16 rows and 68 KB of LDS per workgroup, two per CU -- on an idle masked stream.
                                       // 0: never -- the default: measured SLOWER (round 6: c2 7.8 -> 8.9 ms, c3 50.2 -> 53): at 68 KB a row workgroup shares its CU with an
                                       // update workgroup and runs at half speed; the 152 KB of the one-launch form are what keeps a CU to itself (MEASUREMENTS.md)
  int trsv_resident = 1;               // single right-hand side: one resident launch per direction (trsv.hip); 0: one launch per tile (rounds 1-5)
  // the substitution's panel step that follows the last chain launch through the same flags (panel_chain_v_kernel) ...
  int ride_vchain_pre = 1;             // ... dispatched only once the chain kernel itself can be (ev_chain_pre)
  int ride_vchain_max_wgs = 96;        // ... for right-hand sides of at most this many 32-column workgroups (they wait ON the chip, one per CU; 0: never)
  int ride_same_stream_max_tiles = 0;  // ... on the panel stream itself for factors of at most this many tile rows
  int64_t ride_outer_rows = 2048;      // ... two-level form: rows below an outer block of this many rows are updated once per block (0: every panel updates all rows below) ...
  int ride_outer_min_tiles = 64;       // ... from this many tile rows on
  int ride_max_tiles = 384;            // factors of at least this many tile rows: factorisation and substitution back to back instead (potrf.hip)
  int ride_gate_pct = -1;              // (-1: by size, potrf.hip)              // ... its steps are held back until at most this percentage of the tile rows is left to factor (>= 100: released at once)
  int64_t nb = 512;                // panel width of the blocked Cholesky
  int64_t nb_outer_solve = 4096;   // forward substitution: rows below an outer block of this many rows are updated once per block (two-level scheme, potrf.hip); 0: plain right-looking
  int scoped_gather = 1;           // Pr, Pc > 1 grids: a panel's rows go only to the process row / column whose updates read them (0: to everyone, rounds 1-3)
  int panel_exclusive = 1;         // two-level forward substitution: its panel chains wait for the tail of the long update instead of slipping into it (0: rounds' 4 first behaviour)
  int fused_ahead_min_us = 800;    // ... while the remainder update is estimated at least this long (the fused launch shares its CUs with the update for most of the update's duration)
  int fused_ahead = 1;             // forward substitution: the look-ahead update rides in front of the next fused panel chain (one launch; 0: a launch of its own, rounds 1-3)
  int small_ring2 = 32;            // rank-128 in-panel updates of at least this many 128-tiles run on the two-stage ring of the 64 x 64 kernel (four workgroups per CU); 0: never
  int nb_outer_solve_min_tiles = 384;  // ... from this many tile rows on (c4; measured no gain at c3 / c5 sizes)
  int64_t nb_solve = 0;            // panel width of the blocked forward substitution (0: by size, see trsm_lower_blocked)
  int64_t nb_big = 0;              // optional wider panels while more than nb_big_min_tiles tile rows remain (0 = off; measured: no gain at c3)
  int nb_big_min_tiles = 96;
  int lookahead = 1;
  // estimated duration of one tile step of the panel chain (factorisation / forward substitution) and of
  // the per-panel rest, in microseconds: decides whether the remainder update is released with the panel
  // (update-bound) or after the look-ahead half (chain-bound)
  double chain_us_tile = 150.0, solve_chain_us_tile = 30.0, chain_us_fixed = 80.0;   // (factorisation: re-swept after the tile solves got their refinement step, scratch/sweep_chain.sh; forward substitution: its fused panel chain takes 117 us per 4 tile rows + 65 us of look-ahead update at c3 -- with the factorisation's 150 us per tile row the second half of the c3 prediction held every remainder update back behind its look-ahead half, 100 us of idle update stream per panel: 23.3 -> 22.7 ms, profiles/r03_solve_chain_estimate.txt)
  int min_supertiles = 128;        // GEMM grid: shrink the super-tile edge until there are this many
  int dense_tiles = 1;             // GEMM grid: dense XCD-balanced tile enumeration (0: legacy super-tile dealing)
  int gemm_band = 8;               // GEMM grid: tile rows per band of the dense enumeration (an XCD works on band x 64/band tiles at a time)
  int fused_solve = 1;             // forward substitution: one launch per panel of <= 512 rows (panel_solve_kernel); 0: a tile solve and an update per tile
  int asm_fast = 1;                // per-entry assembly: descriptors of the common shapes (D <= 2, one group, <= 2 parity classes, degrees <= 4) on the specialised kernel (assemble_fast_kernel; bit-identical to the generic one)
  int kron_wide = 1;               // Kronecker expansion with 16-byte stores where the fast extent is even (kron2w_kernel)
  int asm_batch = 1;               // blocks of a block row that share a descriptor are assembled in one launch (assemble.hip: launch_assemble_batch)
  int asm_ct = 4;                  // assemble_fast_kernel: column tiles per workgroup, at most (LPGP_ASM_CT)
  int asm_factors = 0;             // per-entry assembly / matrix-free product: exponentials of Matern dimensions from per-point factors (eval_entries.h);
                                   // +13 % on the kernel, ~4x the rounding noise of the entries (two exps and a product instead of one exp): off by default
  int gemm3_fact = 0;              // ... inside the FACTORISATION only if set: beside the panel chain the third resident workgroup costs the chain what it gains the update (c3: condition phase 33.6 -> 34.1 ms with it, predict phase 22.9 -> 22.6 ms: the forward substitution keeps it)
  double gemm3_margin = 2.0;       // ... and, inside the factorisation / forward substitution, only while the remainder update is estimated to take this many times longer than the panel chain beside it
  int gemm3 = 768;                 // GEMM / SYRK launches (A not transposed) with at least this many 128 x 128 tiles use the three-workgroups-per-CU kernel (gemm3_f64_kernel); 0: never
  int small_tiles_max = 256;       // GEMM launches with at most this many 128x128 tiles use the 64x64-tile kernel
  int dist_bcast = 0;              // panel exchanges as one ncclBroadcast per piece instead of the point-to-point group (LPGP_DIST_COLLECTIVE=bcast)
  double dist_chain_us_comm = 120.0;   // per-panel communication on the chain of a multi-GPU factorisation (diagonal-block broadcast + head gather), for the chain-bound / update-bound decision (LPGP_DIST_CHAIN_US_COMM)
  int split_gather = 1;            // P x 1 grids with look-ahead: gather the next diagonal block's rows first, the rest off the chain
};

// options_from_env: every row whose environment variable is set (a value the row's rule refuses is ignored).  get / set:
// 0, or -2 with lpgp_last_error set (unknown key, refused value, init-only row); doubles read truncated, bools store 0 / 1.
void options_from_env(Options& o);
int option_get(const Options& o, const char* key, int64_t* value);
int option_set(Options& o, const char* key, int64_t value);
// the rows of the table, for tests: their number and the key of row i (nullptr out of range)
int option_count();
const char* option_name(int i);

}  // namespace lpgp
