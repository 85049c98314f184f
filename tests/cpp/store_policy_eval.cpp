// store_policy_eval.cpp -- what the store-policy rules of csrc/scan_plan.hpp make of (output bytes, option "scan_nt_stores"): for every
// line "<out_bytes> <option>" of its input one line
//   one_pass_store_policy  multi_pass_nt_stores  in_aux  scan_aux at dma_aux 18  scan2_aux
// A stand-alone program (plain g++, never loaded into Python): tests/test_store_policies.py holds its units' expected policies
// against these answers.
#include <cstdio>

#include "scan_plan.hpp"

using namespace mi355;

int main()
{
    unsigned long long bytes = 0;
    int option = 0;
    while (scanf("%llu %d", &bytes, &option) == 2) {
        const int p = one_pass_store_policy(bytes, option);
        printf("%d %d %d %d %d\n", p, multi_pass_nt_stores(bytes, option) ? 1 : 0, in_aux(p), scan_aux(18, p), scan2_aux(p));
    }
    return 0;
}
