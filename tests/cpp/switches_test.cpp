// Exercises resql_amd/csrc/switches.h on the host: every reader against the literal value the expression it replaced gave, for an unset
// variable, "0", "1", "2", the empty string, text without a number, a value below the row's range and one above it - and the named
// cases the switches are known to be odd at.  Built and run by tests/test_switches.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "switches.h"

using namespace rsq::sw;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "switches_test: %s failed at line %d\n", #c, __LINE__); failures++; } } while (0)

static const char* const kInputs[8] = {nullptr, "0", "1", "2", "", "abc", "-7", "99999"};      // nullptr: unset
static void put(const char* name, const char* value) { if (value) setenv(name, value, 1); else unsetenv(name); }

template <Id id> static void flagRow() {
    if constexpr (kTable[id].kind == FLAG_ON || kTable[id].kind == FLAG_OFF) {
        // default on: off only for what atoi reads as 0 ("0", "", "abc"); default off: on only for what it reads as non-zero
        static const bool on[8] = {true, false, true, true, false, false, true, true}, off[8] = {false, false, true, true, false, false, true, true};
        for (int i = 0; i < 8; i++) {
            put(kTable[id].name, kInputs[i]);
            const bool got = flag<id>(), want = (kTable[id].kind == FLAG_ON ? on : off)[i];
            if (got != want) { fprintf(stderr, "switches_test: %s input %d reads %d\n", kTable[id].name, i, (int)got); failures++; }
        }
        unsetenv(kTable[id].name);
    }
}

static int intRows = 0;
template <Id id> static void intRow(const long long (&want)[8]) {
    intRows++;
    for (int i = 0; i < 8; i++) {
        put(kTable[id].name, kInputs[i]);
        const long long got = num<id>();
        if (got != want[i]) { fprintf(stderr, "switches_test: %s input %d reads %lld, not %lld\n", kTable[id].name, i, got, want[i]); failures++; }
    }
    unsetenv(kTable[id].name);
}
template <Id id> static void unclampedRow(const long long (&want)[8]) {
    for (int i = 0; i < 8; i++) {
        put(kTable[id].name, kInputs[i]);
        const long long got = unclamped<id>();
        if (got != want[i]) { fprintf(stderr, "switches_test: %s input %d reads %lld unclamped, not %lld\n", kTable[id].name, i, got, want[i]); failures++; }
    }
    unsetenv(kTable[id].name);
}

int main() {
    // ---- the table itself
    CHECK(N_SWITCHES == 31);
    int nInt = 0, nFlag = 0;
    for (const Row& r : kTable) {
        CHECK(strncmp(r.name, "RSQ_", 4) == 0 && r.meaning[0] != 0 && r.when != 0);
        nInt += r.kind == INT || r.kind == INT64 || r.kind == INT64_WITHIN;
        nFlag += r.kind == FLAG_ON || r.kind == FLAG_OFF;
        unsetenv(r.name);
    }
    CHECK(nFlag == 14 && nInt == 15);

    // ---- flags, every row
#define X(name, kind, def, lo, hi, when, meaning) flagRow<name>();
    RSQ_SWITCHES(X)
#undef X
    // (the two default-off ones by name: unset is off, "0" is off, "1" is on)
    CHECK(kTable[RSQ_FORCE_GENERIC].kind == FLAG_OFF && kTable[RSQ_MULTI_GENERAL_MERGE].kind == FLAG_OFF);

    // ---- integers, every row:           unset   "0"  "1"  "2"   ""  "abc" "-7" "99999"
    intRow<RSQ_CHECK_STATS>(             {0,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_JOIN_BITMAP>(             {1,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_JOIN_RANK>(               {1,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_COMPACT>(                 {1,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_GROUP_VALUES_BY_ADDRESS>( {1,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_STAGED>(                  {1,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_AGG_MODE>(                {0,      0,   1,   2,   0,   0,    0,   5});
    intRow<RSQ_LATE_LOADS>(              {1,      0,   1,   2,   0,   0,    0,   2});
    intRow<RSQ_PARTITION>(               {1,      0,   1,   2,   0,   0,    0,   2});
    intRow<RSQ_DEBUG_TAIL>(              {0,      0,   1,   1,   0,   0,    0,   1});
    intRow<RSQ_SCAN_CHAINED>(            {1,      0,   1,   2,   0,   0,   -7,   99999});      // plain atoi, default 1
    intRow<RSQ_DICT_SCANS>(              {0,      0,   1,   2,   0,   0,   -7,   99999});
    intRow<RSQ_DEVICE_TAIL_MIN>(         {65536,  0,   1,   2,   0,   0,   -7,   99999});      // plain atoll, default 65536
    intRow<RSQ_MAX_GRID>(                {0,      0,   1,   2,   0,   0,    0,   0});          // outside 1..65535 reads as 0
    intRow<RSQ_TAIL_THREADS>(            {0,      1,   1,   2,   1,   1,    1,   64});         // unset: 0 = from the hardware; set: 1..64
    CHECK(intRows == nInt);
    // the execution-time reads that never clamped
    unclampedRow<RSQ_PARTITION>(         {1,      0,   1,   2,   0,   0,   -7,   99999});
    unclampedRow<RSQ_DEBUG_TAIL>(        {0,      0,   1,   2,   0,   0,   -7,   99999});

    // ---- RSQ_TRACE: presence switches it on, the value is the level
    {
        static const bool on[8] = {false, true, true, true, true, true, true, true}, two[8] = {false, false, false, true, false, false, false, true};
        static const int lvl[8] = {0, 0, 1, 2, 0, 0, -7, 99999};
        for (int i = 0; i < 8; i++) {
            put("RSQ_TRACE", kInputs[i]);
            const Level l = level<RSQ_TRACE>();
            CHECK(l.on == on[i] && traceOn() == on[i] && l.atLeast(2) == two[i] && (!l.on || l.level == lvl[i]));
        }
        unsetenv("RSQ_TRACE");
    }
    // ---- RSQ_KCACHE_USED_LOG: the text itself
    CHECK(path<RSQ_KCACHE_USED_LOG>() == nullptr);
    setenv("RSQ_KCACHE_USED_LOG", "/tmp/used", 1);
    CHECK(path<RSQ_KCACHE_USED_LOG>() && strcmp(path<RSQ_KCACHE_USED_LOG>(), "/tmp/used") == 0);
    setenv("RSQ_KCACHE_USED_LOG", "", 1);
    CHECK(path<RSQ_KCACHE_USED_LOG>() && path<RSQ_KCACHE_USED_LOG>()[0] == 0);
    unsetenv("RSQ_KCACHE_USED_LOG");

    // ---- the named cases
    setenv("RSQ_TRACE", "0", 1);
    CHECK(traceOn() && level<RSQ_TRACE>().level == 0 && !level<RSQ_TRACE>().atLeast(2));      // RSQ_TRACE=0: tracing on, below level 2
    unsetenv("RSQ_TRACE");
    setenv("RSQ_NARROW_SCANS", "", 1);
    CHECK(!flag<RSQ_NARROW_SCANS>());                                                           // set but empty: off
    unsetenv("RSQ_NARROW_SCANS");
    CHECK(flag<RSQ_NARROW_SCANS>() && !dictScansEnabled() && !dictJoinKeysEnabled());           // nothing set: narrow on, dictionaries off
    setenv("RSQ_DICT_SCANS", "2", 1);
    CHECK(dictScansEnabled() && dictJoinKeysEnabled());
    setenv("RSQ_NARROW_SCANS", "0", 1);
    CHECK(!dictScansEnabled() && !dictJoinKeysEnabled());                                       // RSQ_NARROW_SCANS=0 turns both off
    unsetenv("RSQ_NARROW_SCANS");
    setenv("RSQ_DICT_SCANS", "1", 1);
    CHECK(dictScansEnabled() && !dictJoinKeysEnabled());
    setenv("RSQ_DICT_SCANS", "0", 1);
    CHECK(!dictScansEnabled() && !dictJoinKeysEnabled());
    setenv("RSQ_DICT_SCANS", "-1", 1);
    CHECK(dictScansEnabled() && !dictJoinKeysEnabled());                                        // (atoi != 0, and not >= 2)
    setenv("RSQ_DICT_SCANS", "", 1);
    CHECK(!dictScansEnabled() && !dictJoinKeysEnabled());
    unsetenv("RSQ_DICT_SCANS");
    for (const char* v : {"0", "65536", "-3"}) { setenv("RSQ_MAX_GRID", v, 1); CHECK(num<RSQ_MAX_GRID>() == 0); }
    setenv("RSQ_MAX_GRID", "65535", 1);
    CHECK(num<RSQ_MAX_GRID>() == 65535);
    setenv("RSQ_MAX_GRID", "4294967297", 1);                                                    // (atol, not atoi: this is not 1)
    CHECK(num<RSQ_MAX_GRID>() == 0);
    unsetenv("RSQ_MAX_GRID");
    CHECK(num<RSQ_DEVICE_TAIL_MIN>() == 65536);
    setenv("RSQ_DEVICE_TAIL_MIN", "1", 1);
    CHECK(num<RSQ_DEVICE_TAIL_MIN>() == 1);
    setenv("RSQ_DEVICE_TAIL_MIN", "5000000000", 1);                                             // (atoll)
    CHECK(num<RSQ_DEVICE_TAIL_MIN>() == 5000000000ll);
    unsetenv("RSQ_DEVICE_TAIL_MIN");
    setenv("RSQ_AGG_MODE", "9", 1);
    CHECK(num<RSQ_AGG_MODE>() == 5);
    unsetenv("RSQ_AGG_MODE");
    setenv("RSQ_LATE_LOADS", "-1", 1);
    CHECK(num<RSQ_LATE_LOADS>() == 0);
    unsetenv("RSQ_LATE_LOADS");
    setenv("RSQ_PARTITION", "-1", 1);
    CHECK(num<RSQ_PARTITION>() == 0);
    setenv("RSQ_PARTITION", "3", 1);
    CHECK(num<RSQ_PARTITION>() == 2 && unclamped<RSQ_PARTITION>() == 3);                        // compiled partitioned, not forced at execution (== 2)
    unsetenv("RSQ_PARTITION");
    setenv("RSQ_TAIL_THREADS", "0", 1);
    CHECK(num<RSQ_TAIL_THREADS>() == 1);
    setenv("RSQ_TAIL_THREADS", "100", 1);
    CHECK(num<RSQ_TAIL_THREADS>() == 64);
    unsetenv("RSQ_TAIL_THREADS");
    setenv("RSQ_DEBUG_TAIL", "2", 1);
    CHECK(num<RSQ_DEBUG_TAIL>() == 1 && unclamped<RSQ_DEBUG_TAIL>() == 2);                      // the code generator sees 1, the execution 2
    unsetenv("RSQ_DEBUG_TAIL");

    if (failures) return 1;
    printf("switches_test ok\n");
    return 0;
}
