// switches.h - every environment switch the library reads: one table, one parser, typed readers.  A new switch is a new row here (and a
// row in DESIGN.md §8, and a flip in tests/test_gpu_knobs.py or a test file of its own: tests/test_switch_list.py holds the three together).
// Nothing else in this directory calls getenv.  The long form of what a switch selects is in docs/KERNELS.md and DESIGN.md §8.
#pragma once
#include <cstdlib>

namespace rsq {
namespace sw {

enum Kind {
    FLAG_ON,        // on unless set to something atoi reads as 0 - which includes the empty string and any text without a leading number
    FLAG_OFF,       // off unless set to something atoi reads as non-zero
    INT,            // atoi; unset: the default; set: clamped to [lo, hi]
    INT64,          // the same through atoll
    INT64_WITHIN,   // atoll; unset or outside [lo, hi]: the default
    LEVEL,          // presence switches it on, whatever the value; the value (atoi) is the level
    PATH            // a file name
};
// when the library reads it (a switch flipped later is not seen by what was made before)
enum When { ONCE = 1 /* per process, at first use */, TABLE = 2 /* a table is created or appended to */, COMPILE = 4 /* a statement is compiled */, EXEC = 8 /* every execution */ };

constexpr long long NOLO = -0x7fffffffffffffffLL - 1, NOHI = 0x7fffffffffffffffLL;      // no clamp

//  name, kind, default, lo, hi, read when, meaning
#define RSQ_SWITCHES(X) \
    X(RSQ_POLL,                    FLAG_ON,  1, 0, 1, EXEC,           "0: stream synchronisation instead of polling the sequence number / querying the stream") \
    X(RSQ_PUBLISH_STATUS,          FLAG_ON,  1, 0, 1, EXEC,           "0: status words by copies instead of the kernel that writes them into pinned memory") \
    X(RSQ_FUSED_STEP,              FLAG_ON,  1, 0, 1, EXEC,           "0: the one-launch step as separate launches") \
    X(RSQ_FUSED_SELECT,            FLAG_ON,  1, 0, 1, EXEC,           "0: candidate selection as separate launches") \
    X(RSQ_RANK_CHAINED,            FLAG_ON,  1, 0, 1, EXEC,           "0: rank index in two launches") \
    X(RSQ_SCAN_CHAINED,            INT,      1, NOLO, NOHI, EXEC,     "offset scan in one launch: 0 never, 2 at every size, anything else from 8 M counts on (not clamped)") \
    X(RSQ_DEVICE_TAIL,             FLAG_ON,  1, 0, 1, EXEC,           "0: the tails of large aggregations on the host") \
    X(RSQ_DEVICE_TAIL_MIN,         INT64,    65536, NOLO, NOHI, EXEC, "fewest groups the device tails take (not clamped)") \
    X(RSQ_DEVICE_REPLAY,           FLAG_ON,  1, 0, 1, EXEC,           "0: the replay of the reference's hash table on the host") \
    X(RSQ_DEVICE_TOPK,             FLAG_ON,  1, 0, 1, EXEC,           "0: no candidate pre-selection for ORDER BY ... LIMIT (read by a statement's first execution that could use it)") \
    X(RSQ_MULTI_GENERAL_MERGE,     FLAG_OFF, 0, 0, 1, EXEC,           "1: the general merge although the shards are provably disjoint") \
    X(RSQ_GENERIC,                 FLAG_ON,  1, 0, 1, COMPILE,        "0: blocking compile instead of the interpreter in front") \
    X(RSQ_GENERIC2,                FLAG_ON,  1, 0, 1, COMPILE,        "0: no whole-pipeline interpreter") \
    X(RSQ_FORCE_GENERIC,           FLAG_OFF, 0, 0, 1, COMPILE,        "1: every eligible plan stays on the interpreter") \
    X(RSQ_COMPILE_HELPERS,         FLAG_ON,  1, 0, 1, COMPILE,        "0: kernels compiled in process, one after the other") \
    X(RSQ_CHECK_STATS,             INT,      0, 0, 1, COMPILE,        "1: statistics range checks for engine-owned columns too") \
    X(RSQ_JOIN_BITMAP,             INT,      1, 0, 1, COMPILE,        "0: no key bitmap in front of a join table") \
    X(RSQ_JOIN_RANK,               INT,      1, 0, 1, COMPILE,        "0: the hash form of every join table") \
    X(RSQ_COMPACT,                 INT,      1, 0, 1, COMPILE,        "0: no wave compaction") \
    X(RSQ_GROUP_VALUES_BY_ADDRESS, INT,      1, 0, 1, COMPILE,        "0: string group values that depend on the key are copied into the entries") \
    X(RSQ_STAGED,                  INT,      1, 0, 1, COMPILE,        "0: exact instead of staged partitioning") \
    X(RSQ_AGG_MODE,                INT,      0, 0, 5, COMPILE,        "1-5: force an aggregation sink (5: generic hash aggregation even where a dense id exists)") \
    X(RSQ_LATE_LOADS,              INT,      1, 0, 2, COMPILE,        "0 never / 2 always the late-load form") \
    X(RSQ_PARTITION,               INT,      1, 0, 2, COMPILE | EXEC, "0 never partitions a large dense aggregation, 2 always does.  Quirk: the execution compares the unclamped value with 2, so 3 compiles the partitioned form and does not force it") \
    X(RSQ_DEBUG_TAIL,              INT,      0, 0, 1, COMPILE | EXEC, "1: device timestamps per workgroup.  Quirk: the execution prints more where the unclamped value is >= 2") \
    X(RSQ_NARROW_SCANS,            FLAG_ON,  1, 0, 1, TABLE | COMPILE, "0: no column images are built and no scan reads one.  Quirk of every default-on flag: set but empty is off") \
    X(RSQ_DICT_SCANS,              INT,      0, NOLO, NOHI, TABLE | COMPILE, "non-zero: dictionary images of low-cardinality string columns; >= 2: build-side strings are dense group keys too (dictScansEnabled / dictJoinKeysEnabled below)") \
    X(RSQ_MAX_GRID,                INT64_WITHIN, 0, 1, 65535, COMPILE, "the tile loops launch at most n 256-thread workgroups' worth of threads; 0 = the grid the pipeline asks for") \
    X(RSQ_TAIL_THREADS,            INT,      0, 1, 64, ONCE,          "size of the host worker pool; 0 (unset) = from the hardware") \
    X(RSQ_TRACE,                   LEVEL,    0, 0, 0, COMPILE | EXEC, "phase times on stderr, synchronising after every pipeline; >= 2: host phases of a general execution and of the replay.  Quirk: RSQ_TRACE=0 is on") \
    X(RSQ_KCACHE_USED_LOG,         PATH,     0, 0, 0, COMPILE | EXEC, "file that receives the cache key of every kernel resolved (the build prunes the cache by it)")

enum Id {
#define X(name, kind, def, lo, hi, when, meaning) name,
    RSQ_SWITCHES(X)
#undef X
    N_SWITCHES
};

struct Row { const char* name; Kind kind; long long def, lo, hi; int when; const char* meaning; };
constexpr Row kTable[N_SWITCHES] = {
#define X(name, kind, def, lo, hi, when, meaning) {#name, kind, def, lo, hi, when, meaning},
    RSQ_SWITCHES(X)
#undef X
};

// The parser.  INT rows take the value as atoi would: (int)atoll(e) is what atoi(e) returns wherever long has 64 bits.
struct Parsed { const char* text; long long value; };      // text == nullptr: unset
inline Parsed parse(Id id) {
    const char* e = getenv(kTable[id].name);
    long long v = e ? atoll(e) : 0;
    if (kTable[id].kind != INT64 && kTable[id].kind != INT64_WITHIN) v = (int)v;
    return {e, v};
}

template <Id id> bool flag() {
    static_assert(kTable[id].kind == FLAG_ON || kTable[id].kind == FLAG_OFF, "not a flag");
    const Parsed p = parse(id);
    return kTable[id].kind == FLAG_ON ? !(p.text && p.value == 0) : p.text && p.value != 0;
}
template <Id id> long long num() {
    constexpr Row r = kTable[id];
    static_assert(r.kind == INT || r.kind == INT64 || r.kind == INT64_WITHIN, "not an integer");
    const Parsed p = parse(id);
    if (!p.text) return r.def;
    if (r.kind == INT64_WITHIN) return p.value >= r.lo && p.value <= r.hi ? p.value : r.def;
    return p.value < r.lo ? r.lo : p.value > r.hi ? r.hi : p.value;
}
// ... without the clamp: the two execution-time reads that never had one (RSQ_PARTITION, RSQ_DEBUG_TAIL)
template <Id id> long long unclamped() {
    static_assert(kTable[id].kind == INT || kTable[id].kind == INT64, "not a clamped integer");
    const Parsed p = parse(id);
    return p.text ? p.value : kTable[id].def;
}
struct Level {
    bool on; int level;
    bool atLeast(int n) const { return on && level >= n; }
};
template <Id id> Level level() {
    static_assert(kTable[id].kind == LEVEL, "not a level");
    const Parsed p = parse(id);
    return {p.text != nullptr, (int)p.value};
}
template <Id id> const char* path() {
    static_assert(kTable[id].kind == PATH, "not a path");
    return parse(id).text;
}

inline bool traceOn() { return level<RSQ_TRACE>().on; }
// RSQ_NARROW_SCANS=0 turns the dictionary images off as well
inline bool dictScansEnabled() { return flag<RSQ_NARROW_SCANS>() && num<RSQ_DICT_SCANS>() != 0; }
inline bool dictJoinKeysEnabled() { return flag<RSQ_NARROW_SCANS>() && num<RSQ_DICT_SCANS>() >= 2; }

}  // namespace sw
}  // namespace rsq
