// The table of context options (options.h): one row per option, and the three walkers over it -- the environment at
// lpgp_init, lpgp_get_option and lpgp_set_option.  The defaults are the initialisers of lpgp::Options.
#include "options.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "lpgp_desc.h"

namespace lpgp {
namespace {

enum class Kind { Int, Int64, Double, Bool };   // Bool: an int field that holds 0 / 1

// the kind of a row, checked against the type of its field (a mismatch does not compile: the table is constexpr)
template <class T>
constexpr Kind kind_of(Kind k) {
  return (std::is_same<T, int>::value && (k == Kind::Int || k == Kind::Bool)) || (std::is_same<T, int64_t>::value && k == Kind::Int64) ||
         (std::is_same<T, double>::value && k == Kind::Double) ? k : throw "option kind does not match its field";
}

// validity rule: `ok` (nullptr: every value) and the message of a refused value (printf format; %d: `arg`)
struct Rule { bool (*ok)(int64_t); const char* refusal; int arg; };
constexpr Rule ANY{nullptr, nullptr, 0};
constexpr Rule tiles(const char* refusal) { return {[](int64_t v) { return v >= 0 && v % TILE == 0; }, refusal, TILE}; }

struct Row {
  const char* key;
  const char* env;      // nullptr: none
  Kind kind;
  size_t off;           // of the field in Options
  Rule rule;
  bool init_only;       // read from the environment at lpgp_init only: set refuses it
};

#define OPT(field, env, kind, ...) Row{#field, env, kind_of<decltype(Options::field)>(Kind::kind), offsetof(Options, field), __VA_ARGS__}

constexpr Row kRows[] = {
    // streams (lpgp_init)
    OPT(reserve_cus, "LPGP_RESERVE_CUS", Int, ANY, true),
    OPT(reserve_narrow, "LPGP_RESERVE_CUS_NARROW", Int, ANY, true),
    OPT(single_stream, "LPGP_SINGLE_STREAM", Bool, ANY, true),
    // blocked Cholesky
    OPT(nb, "LPGP_NB", Int64, {[](int64_t v) { return v >= TILE && v % TILE == 0; }, "nb must be a positive multiple of %d", TILE}, false),
    OPT(lookahead, "LPGP_LOOKAHEAD", Bool, ANY, false),
    OPT(nb_outer, "LPGP_NB_OUTER", Int64, tiles("nb_outer must be a multiple of %d (0 disables)"), false),
    OPT(nb_outer_min_tiles, "LPGP_NB_OUTER_MIN_TILES", Int, ANY, false),
    OPT(nb_big, "LPGP_NB_BIG", Int64, tiles("nb_big must be a multiple of %d (0 disables)"), false),
    OPT(nb_big_min_tiles, "LPGP_NB_BIG_MIN_TILES", Int, ANY, false),
    OPT(chain_us_tile, "LPGP_CHAIN_US_TILE", Double, ANY, false),
    OPT(chain_us_fixed, "LPGP_CHAIN_US_FIXED", Double, ANY, false),
    OPT(chain_resident_max_rows, "LPGP_CHAIN_RESIDENT", Int, ANY, false),
    OPT(chain_resident2_max_rows, "LPGP_CHAIN_RESIDENT2", Int, ANY, false),
    OPT(chain_ahead, "LPGP_CHAIN_AHEAD", Bool, ANY, false),
    OPT(chain_ahead_min_rows, "LPGP_CHAIN_AHEAD_MIN_ROWS", Int, ANY, false),
    OPT(append_split, "LPGP_APPEND_SPLIT", Bool, ANY, false),
    OPT(append_split_min_tiles, "LPGP_APPEND_SPLIT_MIN_TILES", Int, ANY, false),
    // forward substitution
    OPT(nb_solve, "LPGP_NB_SOLVE", Int64, tiles("nb_solve must be a multiple of %d (0: nb)"), false),
    OPT(nb_outer_solve, "LPGP_NB_OUTER_SOLVE", Int64, tiles("nb_outer_solve must be a multiple of %d (0 disables)"), false),
    OPT(nb_outer_solve_min_tiles, "LPGP_NB_OUTER_SOLVE_MIN_TILES", Int, {[](int64_t v) { return v >= 0; }, "nb_outer_solve_min_tiles must be >= 0", 0}, false),
    OPT(solve_chain_us_tile, "LPGP_SOLVE_CHAIN_US_TILE", Double, ANY, false),
    OPT(fused_solve, "LPGP_FUSED_SOLVE", Bool, ANY, false),
    OPT(fused_ahead, "LPGP_FUSED_AHEAD", Int, ANY, false),
    OPT(fused_ahead_min_us, "LPGP_FUSED_AHEAD_MIN_US", Int, ANY, false),
    OPT(panel_exclusive, "LPGP_PANEL_EXCLUSIVE", Bool, ANY, false),
    OPT(trsv_resident, "LPGP_TRSV_RESIDENT", Bool, ANY, false),
    // factorisation with the substitution riding along (potrf_predict_blocked)
    OPT(ride_stream, "LPGP_RIDE_STREAM", Int, ANY, false),
    OPT(ride_occ3, "LPGP_RIDE_OCC3", Bool, ANY, false),
    OPT(ride_aug, "LPGP_RIDE_AUG", Int, ANY, false),
    OPT(ride_b_on_ride, "LPGP_RIDE_B_ON_RIDE", Bool, ANY, false),
    OPT(ride_old_ungated, "LPGP_RIDE_OLD_UNGATED", Bool, ANY, false),
    OPT(ride_vchain_pre, "LPGP_RIDE_VCHAIN_PRE", Bool, ANY, false),
    OPT(ride_vchain_max_wgs, "LPGP_RIDE_VCHAIN", Int, ANY, false),
    OPT(ride_gate_pct, "LPGP_RIDE_GATE_PCT", Int, ANY, false),
    OPT(ride_outer_rows, "LPGP_RIDE_OUTER_ROWS", Int64, {[](int64_t v) { return v >= 0 && v % (4 * TILE) == 0; }, "ride_outer_rows must be a multiple of %d (0 disables)", 4 * TILE}, false),
    OPT(ride_outer_min_tiles, "LPGP_RIDE_OUTER_MIN_TILES", Int, ANY, false),
    OPT(ride_max_tiles, "LPGP_RIDE_MAX_TILES", Int, ANY, false),
    OPT(ride_same_stream_max_tiles, "LPGP_RIDE_SAME_STREAM_MAX_TILES", Int, ANY, false),
    // GEMM / SYRK
    OPT(gemm3, "LPGP_GEMM3", Int, ANY, false),     // (set: negative restores the default)
    OPT(gemm3_fact, "LPGP_GEMM3_FACT", Bool, ANY, false),
    OPT(gemm3_margin, "LPGP_GEMM3_MARGIN", Double, ANY, false),
    OPT(small_tiles_max, "LPGP_SMALL_TILES_MAX", Int, ANY, false),
    OPT(small_ring2, "LPGP_SMALL_RING2", Int, ANY, false),
    OPT(min_supertiles, nullptr, Int, ANY, false),
    OPT(dense_tiles, "LPGP_DENSE_TILES", Bool, ANY, false),
    OPT(gemm_band, "LPGP_GEMM_BAND", Int, {[](int64_t v) { return v == 2 || v == 4 || v == 8 || v == 16 || v == 32; }, "gemm_band must be one of 2, 4, 8, 16, 32", 0}, false),
    // assembly
    OPT(asm_fast, "LPGP_ASM_FAST", Bool, ANY, false),
    OPT(asm_ct, "LPGP_ASM_CT", Int, {[](int64_t v) { return v >= 1 && v <= 64; }, "asm_ct must be in 1 .. 64", 0}, false),
    OPT(asm_batch, "LPGP_ASM_BATCH", Bool, ANY, false),
    OPT(asm_factors, "LPGP_ASM_FACTORS", Bool, ANY, false),
    OPT(kron_wide, "LPGP_KRON_WIDE", Bool, ANY, false),
    // multi-GPU (the same on every rank)
    OPT(dist_bcast, "LPGP_DIST_COLLECTIVE", Bool, ANY, false),     // (env: 1 only for "bcast")
    OPT(split_gather, "LPGP_DIST_SPLIT_GATHER", Bool, ANY, false),
    OPT(scoped_gather, "LPGP_DIST_SCOPED_GATHER", Bool, ANY, false),
    OPT(dist_chain_us_comm, "LPGP_DIST_CHAIN_US_COMM", Double, ANY, false),
};
#undef OPT

const Row* find(const char* key) {
  for (const Row& r : kRows)
    if (key && std::strcmp(r.key, key) == 0) return &r;
  return nullptr;
}

template <class T>
T& field(Options& o, const Row& r) { return *reinterpret_cast<T*>(reinterpret_cast<char*>(&o) + r.off); }
template <class T>
const T& field(const Options& o, const Row& r) { return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(&o) + r.off); }

int64_t load(const Options& o, const Row& r) {
  switch (r.kind) {
    case Kind::Int64: return field<int64_t>(o, r);
    case Kind::Double: return (int64_t)field<double>(o, r);
    default: return field<int>(o, r);
  }
}

void store(Options& o, const Row& r, int64_t v) {
  switch (r.kind) {
    case Kind::Int: field<int>(o, r) = (int)v; break;
    case Kind::Bool: field<int>(o, r) = v != 0; break;
    case Kind::Int64: field<int64_t>(o, r) = v; break;
    case Kind::Double: field<double>(o, r) = (double)v; break;
  }
}

bool valid(const Row& r, int64_t v) { return !r.rule.ok || r.rule.ok(v); }

}  // namespace

void options_from_env(Options& o) {
  for (const Row& r : kRows) {
    const char* e = r.env ? std::getenv(r.env) : nullptr;
    if (!e) continue;
    if (r.kind == Kind::Double) {
      field<double>(o, r) = std::atof(e);
    } else {
      const int64_t v = std::strcmp(r.key, "dist_bcast") == 0 ? std::strcmp(e, "bcast") == 0 : std::atoll(e);
      if (valid(r, v)) store(o, r, v);      // (a value the row refuses is ignored: the default stays)
    }
  }
  // A profiler that SERIALISES kernels (rocprofv3 --pmc / counter groups: ROCPROF_COUNTER_COLLECTION) breaks the one assumption of
  // the follower -- that its chain kernel is dispatched beside it: it would wait out its poll limit, ~1 s per panel, and the step
  // would fail with a negative status.  Off there unless asked for explicitly.
  const char* e = std::getenv("ROCPROF_COUNTER_COLLECTION");
  if (e && e[0] != '\0' && e[0] != '0' && e[0] != 'F' && e[0] != 'f' && !std::getenv("LPGP_RIDE_VCHAIN")) o.ride_vchain_max_wgs = 0;
}

int option_get(const Options& o, const char* key, int64_t* value) {
  const Row* r = find(key);
  LPGP_CHECK(r, "unknown option %s", key ? key : "");
  *value = load(o, *r);
  return 0;
}

int option_set(Options& o, const char* key, int64_t value) {
  const Row* r = find(key);
  LPGP_CHECK(r, "unknown option %s", key ? key : "");
  LPGP_CHECK(!r->init_only, "%s is read at lpgp_init only (environment variable %s)", key, r->env);
  if (std::strcmp(key, "gemm3") == 0 && value < 0) value = Options().gemm3;      // (negative: back to the built-in default)
  LPGP_CHECK(valid(*r, value), r->rule.refusal, r->rule.arg);
  store(o, *r, value);
  return 0;
}

int option_count() { return (int)(sizeof(kRows) / sizeof(kRows[0])); }
const char* option_name(int i) { return i >= 0 && i < option_count() ? kRows[i].key : nullptr; }

}  // namespace lpgp
