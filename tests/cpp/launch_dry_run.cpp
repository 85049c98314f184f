// launch_dry_run.cpp -- what the width-group launchers WOULD launch, without a GPU (tests/test_launch_plan.py).
//
// Links against csrc/build/width_group_*.o.  Every request carries LaunchReq::choice_out, so nothing is launched: the
// launchers only decide, report the kernel family and write the launch-record line.  The occupancy queries have no device
// to ask and fall back to one block per CU, so the grid column means nothing here.
//
// stdin, one case per line:  op c P layout hits n kernel_flags shared_vpl scan_nt_stores max_blocks_per_cu dma_aux scan_burst select_single
//   [llc_resident_mib llc_repeat]
//   (kernel_flags: the option as a caller sets it; it goes through kernel_switch_word() as in capi.hip's launch(); without the two
//   trailing columns the Infinity Cache option is auto and the call no repeat, so the divisor is 0)
// stdout, one line per case: <family or -1> TAB <launch record line>; with the trailing columns also TAB <the Infinity Cache divisor
//   the launcher chose (LaunchReq::llc_d_out), -1 = the op reports none>
// --switches: the table of switches.hpp instead, one row per line: name TAB option value TAB kernel bit TAB receiver
#include <cstdio>
#include <cstring>
#include <string>

#include "dispatch.hpp"

using namespace mi355;

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--switches")) {
        for (const SwitchRow &s : kSwitches) printf("%s\t%u\t0x%x\t%s\n", s.name, s.option, s.kbit, kSwitchReceiverName[s.receiver]);
        return 0;
    }
    hipError_t (*const groups[kNumGroups])(const LaunchReq &) = MI355_GROUP_TABLE(launch_group_);
    int op, layout, hits, shared_vpl, nts, max_bpc, dma_aux, burst, single;
    unsigned c, P, flags;
    unsigned long long n, dummy = 0;
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        int llc_mib = -1, llc_repeat = 0, llc_d = -1;
        const int fields = sscanf(line, "%d %u %u %d %d %llu %u %d %d %d %d %d %d %d %d", &op, &c, &P, &layout, &hits, &n, &flags, &shared_vpl, &nts,
                                  &max_bpc, &dma_aux, &burst, &single, &llc_mib, &llc_repeat);
        if (fields == EOF) continue; // a blank line
        if ((fields != 13 && fields != 15) || c < 1 || c > 32) return 2;
        std::string record;
        int family = -1;
        LaunchReq r{};
        r.op = op;
        r.c = c;
        r.num_cus = 256;
        r.max_blocks_per_cu = max_bpc;
        r.dma_aux = dma_aux;
        r.scan_nt_stores = nts;
        r.scan_burst = burst;
        r.llc_resident_mib = llc_mib;
        r.llc_repeat = llc_repeat;
        r.llc_d_out = &llc_d;
        r.select_single = single;
        r.shared_vpl = shared_vpl;
        r.record = &record;
        r.choice_out = &family;
        r.scan.n = n;
        r.scan.nkeys = P;
        r.scan.layout = (uint32_t)layout;
        r.scan.hits = hits ? &dummy : nullptr;
        r.scan.flags = kernel_switch_word(flags, op == kOpSelect);
        r.decomp.n = n;
        const hipError_t e = groups[(c - 1) / 4](r);
        if (e != hipSuccess) {
            fprintf(stderr, "op %d c %u P %u: %s\n", op, c, P, hipGetErrorString(e));
            return 1;
        }
        if (!record.empty() && record.back() == '\n') record.pop_back();
        if (fields == 15)
            printf("%d\t%s\t%d\n", family, record.c_str(), llc_d);
        else
            printf("%d\t%s\n", family, record.c_str());
    }
    return 0;
}
