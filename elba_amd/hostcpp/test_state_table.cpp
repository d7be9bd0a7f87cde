// test_state_table — walks csrc/state.hpp's table without the library: every argument is an event name, optionally suffixed
// ":reject" or ":state" (the call is refused for its arguments / for what the context holds: only `enter` applies) or ":fail" (it
// fails after its checks have passed: `enter` and `accepted`).
// Prints one line per event: the event as given, the mask in hex, the valid products by name (tests/test_state_cpu.py reads them).
#include "../csrc/state.hpp"
#include <cstdio>
#include <cstring>
#include <string>

using namespace elba;

static const char *const PRODUCT_NAMES[P_COUNT] = {"reads", "counts", "A", "B", "aln", "edges", "S", "contigs", "pileup", "trim"};

// the four calls that change S in place share one row: what elba_clip_tips does to a context, the other three do
constexpr bool same_row(Event a, Event b)
{
    return TABLE[a].enter == TABLE[b].enter && TABLE[a].accepted == TABLE[b].accepted && TABLE[a].done == TABLE[b].done && TABLE[a].publish == TABLE[b].publish &&
           TABLE[a].of_aln == TABLE[b].of_aln;
}
static_assert(same_row(EV_CLIP_TIPS, EV_POP_BUBBLES) && same_row(EV_CLIP_TIPS, EV_CUT_WEAK_OVERLAPS) && same_row(EV_CLIP_TIPS, EV_CUT_BRIDGES),
              "state.hpp: pop_bubbles, cut_weak_overlaps and cut_bridges are clip_tips, row for row");
static_assert(EV_POP_BUBBLES == EV_CLIP_TIPS + 1 && EV_CUT_WEAK_OVERLAPS == EV_POP_BUBBLES + 1 && EV_CUT_BRIDGES == EV_CUT_WEAK_OVERLAPS + 1,
              "state.hpp: the four rows follow one another");
// the fifth, resolve_stars, is the same row again and stands in front of the four
static_assert(same_row(EV_CLIP_TIPS, EV_RESOLVE_STARS) && EV_RESOLVE_STARS == EV_TRANSITIVE_REDUCTION + 1 && EV_CLIP_TIPS == EV_RESOLVE_STARS + 1,
              "state.hpp: resolve_stars is clip_tips, row for row, between transitive_reduction and clip_tips");

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--events")) {
        for (const Row &r : TABLE) printf("%s\n", r.name);
        return 0;
    }
    Validity v;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a], name = arg.substr(0, arg.find(':')), how = arg.size() > name.size() ? arg.substr(name.size() + 1) : "";
        const Row *row = nullptr;
        for (const Row &r : TABLE) if (name == r.name) row = &r;
        const bool refused = how == "reject" || how == "state";
        if (!row || (how != "" && !refused && how != "fail")) { fprintf(stderr, "test_state_table: unknown event or ending '%s'\n", argv[a]); return 2; }
        enter(v, row->ev);
        if (!refused) accepted(v, row->ev);
        if (how == "") done(v, row->ev);
        printf("%s 0x%03x", argv[a], (unsigned)v.bits);
        for (unsigned p = 0; p < P_COUNT; ++p) if (has(v, (Product)p)) printf(" %s", PRODUCT_NAMES[p]);
        printf("\n");
    }
    return 0;
}
