// pool_groups_plan_check.cpp -- the inverted index, the cut of long lists and the packing of small tables of the pool of a set
// by label (kpal_amd/csrc/pool_groups_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each,
// and knows no expected value -- those are the literals of tests/test_pool_groups_plan_host.py.  Every answer is a line of
// integers.
//   sizes                            -> kPoolGroupsMaxIndex kPoolGroupsMaxGridY kPoolGroupsFinalUnroll
//   ct       TABLES BINS NUM_CU      -> pool_groups_chunk_tables
//   chunks   MEMBERS CHUNK_TABLES    -> pool_groups_chunks
//   lanes    BINS                    -> pool_groups_lane_shift pool_groups_items_per_workgroup
//   iwg      ITEMS BINS              -> pool_groups_item_workgroups
//   fit      TABLES GROUPS BINS      -> pool_groups_fit
//   pscratch CUT ITEMS BINS          -> pool_groups_scratch_bytes
//   labels   BINS NUM_CU GROUPS L..  -> the plan of the labels L.. (signed): status bad_table cut items members chunk_tables
//                                       scratch_bytes, then every word of the index
//   pattern  NAME N GROUPS BINS NUM_CU -> the plan of N labels made here: status bad_table cut items members chunk_tables
//                                       scratch_bytes index_bytes, the shortest non-empty and the longest list of a first-pass
//                                       item, the empty ones, and 1 if the index is sound (see `sound`), else 0
//            NAME: one (every table in group 0), each (table t in group t), skew (table t in group 0 unless t % 10 == 0, then
//            in group 1 + t / 10), mod (table t in group t % GROUPS), last (as one, the last table in group GROUPS)
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../kpal_amd/csrc/pool_groups_plan.hpp"

using namespace kpal;

// Every first-pass item lists tables of ONE group in ascending order, the items of a group follow each other and cover its
// tables once, in ascending order over the whole group; with a cut group g owns the items [group_begin[g], group_begin[g + 1]).
static int sound(const PoolGroupsPlan &p, const std::vector<int64_t> &labels)
{
    const uint32_t *members = p.index.data() + p.members_at(), *begin = p.index.data() + p.begin_at();
    if (p.index.size() != p.members + p.items + 1 + (p.cut ? p.n_groups + 1 : 0)) return 0;
    if (begin[0] != 0 || begin[p.items] != p.members) return 0;
    std::vector<uint64_t> seen(p.n_groups, 0), want(p.n_groups, 0);
    std::vector<int64_t> last(p.n_groups, -1);
    for (int64_t l : labels)
        if (l >= 0) ++want[(size_t)l];
    int64_t group_before = -1;
    for (uint64_t i = 0; i < p.items; ++i) {
        if (begin[i] > begin[i + 1]) return 0;
        if (p.cut && begin[i] == begin[i + 1]) return 0;   // a chunk is never empty
        if (begin[i + 1] - begin[i] > p.chunk_tables && p.cut) return 0;
        int64_t g = p.cut ? -1 : (int64_t)i;
        for (uint32_t m = begin[i]; m < begin[i + 1]; ++m) {
            const uint32_t t = members[m];
            if (t >= labels.size() || labels[t] < 0) return 0;
            if (g < 0) g = labels[t];
            if (labels[t] != g || (int64_t)t <= last[(size_t)g]) return 0;
            last[(size_t)g] = t;
            ++seen[(size_t)g];
        }
        if (g < group_before) return 0;
        group_before = g;
        if (p.cut) {
            const uint32_t *gb = p.index.data() + p.group_begin_at();
            if (!(gb[g] <= i && i < gb[g + 1])) return 0;
        }
    }
    if (p.cut) {
        const uint32_t *gb = p.index.data() + p.group_begin_at();
        if (gb[0] != 0 || gb[p.n_groups] != p.items) return 0;
        for (uint64_t g = 0; g < p.n_groups; ++g)
            if (gb[g + 1] - gb[g] != pool_groups_chunks(want[g], p.chunk_tables)) return 0;
    }
    for (uint64_t g = 0; g < p.n_groups; ++g)
        if (seen[g] != want[g]) return 0;
    return 1;
}

static void head(int status, const PoolGroupsPlan &p)
{
    printf("%d %" PRId64 " %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, status, p.bad_table, p.cut ? 1 : 0, p.items, p.members, p.chunk_tables,
           p.scratch_bytes);
}

int main()
{
    static char line[1 << 16];
    char what[16];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[4] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        if (!strcmp(what, "labels")) {
            char *s = line + at;
            std::vector<int64_t> v;
            for (;;) {
                char *end = nullptr;
                const long long x = strtoll(s, &end, 10);
                if (end == s) break;
                v.push_back(x);
                s = end;
            }
            if (v.size() < 4) {
                printf("bad query: %s", line);
                return 1;
            }
            const std::vector<int64_t> labels(v.begin() + 3, v.end());
            PoolGroupsPlan p;
            const int status = pool_groups_plan(labels.data(), labels.size(), (uint64_t)v[2], (uint64_t)v[0], (uint64_t)v[1], p);
            head(status, p);
            if (status == kPoolGroupsOk)
                for (uint32_t w : p.index) printf(" %u", w);
            printf("\n");
            ++answered;
            continue;
        }
        if (!strcmp(what, "pattern")) {
            char name[16];
            unsigned long long n = 0, groups = 0, bins = 0, cu = 0;
            if (sscanf(line + at, "%15s %llu %llu %llu %llu", name, &n, &groups, &bins, &cu) != 5) {
                printf("bad query: %s", line);
                return 1;
            }
            std::vector<int64_t> labels((size_t)n);
            for (uint64_t t = 0; t < n; ++t) {
                if (!strcmp(name, "one")) labels[t] = 0;
                else if (!strcmp(name, "each")) labels[t] = (int64_t)t;
                else if (!strcmp(name, "skew")) labels[t] = t % 10 != 0 ? 0 : (int64_t)(1 + t / 10);
                else if (!strcmp(name, "mod")) labels[t] = (int64_t)(t % groups);
                else if (!strcmp(name, "last")) labels[t] = t + 1 == n ? (int64_t)groups : 0;
                else {
                    printf("bad query: %s", line);
                    return 1;
                }
            }
            PoolGroupsPlan p;
            const int status = pool_groups_plan(labels.data(), n, groups, bins, cu, p);
            head(status, p);
            uint64_t lo = UINT64_MAX, hi = 0, empty = 0;
            if (status == kPoolGroupsOk) {
                const uint32_t *begin = p.index.data() + p.begin_at();
                for (uint64_t i = 0; i < p.items; ++i) {
                    const uint64_t len = begin[i + 1] - begin[i];
                    if (len == 0) ++empty;
                    else lo = len < lo ? len : lo;
                    hi = len > hi ? len : hi;
                }
            }
            printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n", p.index_bytes(), lo == UINT64_MAX ? 0 : lo, hi, empty,
                   status == kPoolGroupsOk ? sound(p, labels) : 0);
            ++answered;
            continue;
        }
        const int got = sscanf(line + at, "%llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3]);
        if (!strcmp(what, "sizes") && got < 1) printf("%" PRIu64 " %u %d\n", kPoolGroupsMaxIndex, kPoolGroupsMaxGridY, kPoolGroupsFinalUnroll);
        else if (!strcmp(what, "ct") && got == 3) printf("%" PRIu64 "\n", pool_groups_chunk_tables(a[0], a[1], a[2]));
        else if (!strcmp(what, "chunks") && got == 2) printf("%" PRIu64 "\n", pool_groups_chunks(a[0], a[1]));
        else if (!strcmp(what, "lanes") && got == 1) printf("%d %" PRIu64 "\n", pool_groups_lane_shift(a[0]), pool_groups_items_per_workgroup(a[0]));
        else if (!strcmp(what, "iwg") && got == 2) printf("%" PRIu64 "\n", pool_groups_item_workgroups(a[0], a[1]));
        else if (!strcmp(what, "fit") && got == 3) printf("%d\n", pool_groups_fit(a[0], a[1], a[2]) ? 1 : 0);
        else if (!strcmp(what, "pscratch") && got == 3) printf("%" PRIu64 "\n", pool_groups_scratch_bytes(a[0] != 0, a[1], a[2]));
        else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("POOL_GROUPS_PLAN_DONE %d\n", answered);
    return 0;
}
