// Stand-alone check of csrc/group_form.h, the form of a group launch as a pure decision (tests/test_group_form_host.py builds
// it with the host sanitizers): the thresholds in force and every combination of launches in flight 0..4, other groups on the
// device 0..4, both counting forms, fold enabled and disabled.
#include <stdio.h>

#include "../../minorseq_amd/csrc/group_form.h"

static int g_fail = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("FAIL line %d: %s\n", __LINE__, #c);              \
            ++g_fail;                                                \
        }                                                            \
    } while (0)

int main()
{
    // the thresholds in force: a launch from the planes folds below three launches in flight, one from the index only alone
    CHECK(JL_GROUP_FOLD_BELOW == 3u);
    CHECK(JL_GROUP_FOLD_BELOW_INDEX == 1u);
    CHECK(JL_FORM_FOLDED == 0 && JL_FORM_UNFOLDED == 1);   // (a graph's index is form | 2 x index)
    unsigned cases = 0;
    for (uint32_t busy = 0; busy <= 4; ++busy)
        for (uint32_t others = 0; others <= 4; ++others)
            for (int ix = 0; ix < 2; ++ix)
                for (int fold = 0; fold < 2; ++fold) {
                    const jl_group_form_choice c = jl_group_form_decide(busy, others, ix != 0, fold != 0);
                    ++cases;
                    if (!fold) {   // JL_NO_FOLD_CALL: unfolded everywhere, and no folded graph is ever wanted
                        CHECK(c.form == JL_FORM_UNFOLDED);
                        CHECK(!c.other_reachable);
                        continue;
                    }
                    const uint32_t below = ix ? 1u : 3u;
                    const bool folded = ix ? busy == 0u : busy < 3u;
                    CHECK(c.form == (folded ? JL_FORM_FOLDED : JL_FORM_UNFOLDED));
                    // the form not taken: the unfolded one needs `below` other groups to be found in flight, the folded one nobody
                    const bool reachable = folded ? others >= below : true;
                    CHECK(c.other_reachable == reachable);
                    if (c.form != (folded ? JL_FORM_FOLDED : JL_FORM_UNFOLDED) || c.other_reachable != reachable)
                        printf("  at in flight %u, other groups %u, index %d\n", busy, others, ix);
                }
    CHECK(cases == 5u * 5u * 2u * 2u);
    // the cases the set-up launches of a stream of index-form launches rest on: alone on the device, nothing else to capture;
    // one neighbour, the unfolded index graph is captured beside the folded one, the unfolded plane graph is not
    CHECK(!jl_group_form_decide(0, 0, true, true).other_reachable);
    CHECK(jl_group_form_decide(0, 1, true, true).other_reachable);
    CHECK(!jl_group_form_decide(0, 1, false, true).other_reachable && !jl_group_form_decide(0, 2, false, true).other_reachable);
    CHECK(jl_group_form_decide(0, 3, false, true).other_reachable);
    // one launch in flight: the counting forms part
    CHECK(jl_group_form_decide(1, 4, false, true).form == JL_FORM_FOLDED);
    CHECK(jl_group_form_decide(1, 4, true, true).form == JL_FORM_UNFOLDED);
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("ok %u cases\n", cases);
    return 0;
}
