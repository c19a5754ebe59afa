// group_form.h — the form of a group launch (capi_group.hip "Two forms"): a pure decision, host only, so that a stand-alone program
// can check it (tests/cpp/group_form_check.cpp).  FOLDED: the Fisher stage in the counting launch's epilogue; UNFOLDED: the plain
// counting launch + call_group_kernel.  A launch is folded while fewer than a threshold of the device's OTHER group launches are
// incomplete at enqueue time (0: never, a large value: always), and the threshold depends on what the launch counts from:
//   * the planes (JL_GROUP_FOLD_BELOW = 3): a 140 us stream whose epilogue is 1 % of it — the fold pays until three other
//     launches' pileups want the workgroup slots the epilogue holds;
//   * the deviation index (JL_GROUP_FOLD_BELOW_INDEX = 1): a 60 us latency-bound list walk that lives on eight waves per SIMD;
//     the epilogue's registers leave it five (JL_IX_FOLD_WAVES, kernels_pileup.hip; three before that budget), so the fold pays
//     only where nothing else can fill the device: a launch that is ALONE, whose tail is exposed whole.  (Not 0: a lone launch's
//     tail is one launch and one read-back shorter folded.)
// Measured, not guessed: the sweeps are in profiles/ (DESIGN.md "What bounds a step", "With the deviation index").
#pragma once
#include <stdint.h>

#ifndef JL_GROUP_FOLD_BELOW
#define JL_GROUP_FOLD_BELOW 3u
#endif
#ifndef JL_GROUP_FOLD_BELOW_INDEX
#define JL_GROUP_FOLD_BELOW_INDEX 1u
#endif
enum { JL_FORM_FOLDED = 0, JL_FORM_UNFOLDED = 1 };

struct jl_group_form_choice {
    int form;               // JL_FORM_FOLDED / JL_FORM_UNFOLDED: what this launch takes
    bool other_reachable;   // the form NOT taken is one a later launch of this group can take: worth a captured graph now
};

// others_in_flight: the device's other group launches that are incomplete now; other_groups: the other groups that live on the
// device (a launch can only ever find that many in flight); index_form: the launch counts from the deviation index;
// fold_enabled: false under JL_NO_FOLD_CALL — unfolded everywhere, and nothing else reachable.
static inline jl_group_form_choice jl_group_form_decide(uint32_t others_in_flight, uint32_t other_groups, bool index_form, bool fold_enabled)
{
    const uint32_t below = index_form ? (uint32_t)JL_GROUP_FOLD_BELOW_INDEX : (uint32_t)JL_GROUP_FOLD_BELOW;
    if (!fold_enabled || below == 0u) return {JL_FORM_UNFOLDED, false};
    if (others_in_flight < below) return {JL_FORM_FOLDED, other_groups >= below};   // unfolded needs `below` others in flight
    return {JL_FORM_UNFOLDED, true};                                                 // folded needs nobody else
}
