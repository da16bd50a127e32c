// step_end_plan.h -- the pure parts of the end of a Metropolis step: how its event sum and its clearing are cut into
// workgroups, what its kernels ask of LDS, and where the words of a group's `d_ticket` block stand.  Plain C++ with no
// device call, so that a stand-alone program can include it (tests/cpp/test_step_end_plan.cpp); the kernels and their
// launchers (step_end_kernels.inc.h) and the host's rules (sxmc_group.cpp, sxmc_multigroup.cpp) read the same figures.
#pragma once

#include <algorithm>
#include <cstddef>

namespace sxstep {

// The event sum of a step is cut into blocks of kStepSumRows rows (eval_nll_kernel's workgroups: 128 lanes, two waves), and
// the one-workgroup step end (tail_step_kernel) is taken for at most kTailMaxLookups look-ups, rows x members -- so for at
// most two such blocks, whose waves' sums it adds block by block.  One pair of constants for the host's rules
// (step_sum_blocks, step_end_takes_tail) and the kernel that depends on them.
constexpr unsigned kStepSumRows = 128;
constexpr unsigned long long kTailMaxLookups = 256;
static_assert(kTailMaxLookups <= 2 * kStepSumRows, "tail_step_kernel adds the waves' sums of at most two blocks of the event sum");
// The cooperative step ends hand their partial sums over through one slot per worker, polled by one lane of the finisher
// each: at most as many workers as the finisher has lanes (and as a group has slots).
constexpr int kCoopMaxWorkers = 128;

// workgroups of kStepSumRows rows the event sum of a step is cut into (eval_nll_kernel; eval_nll2_kernel per candidate)
inline int step_sum_blocks(unsigned long long ne) {
  return (int)std::min<unsigned long long>(1024, std::max<unsigned long long>(1, (ne + kStepSumRows - 1) / kStepSumRows));
}

// chunks the clearing of one histogram of at most max_bins counters is cut into: 16-byte stores, one per lane of a
// workgroup of `block` lanes and round (clear_piece)
inline int zero_blocks(int max_bins, int block, int most = 1024) {
  return std::min(most, std::max(1, (max_bins / 4 + block - 1) / block));
}

// Dynamic LDS of a kernel that runs eval_nll_block_part over nsig members: 16 wave sums, then the members' staged
// records (EvalMember, kEvalMemberBytes each) in whole passes of 16.
constexpr size_t kEvalMemberBytes = 48;
inline size_t step_end_lds_bytes(size_t nsig) { return 16 * sizeof(double) + (nsig + 15) / 16 * 16 * kEvalMemberBytes; }

// The words of a group's d_ticket block (unsigned each; zeroed at creation and after a timeout).
enum TicketWord : unsigned {
  kTicket = 0,      // arrival counter of the ticket form (eval_nll_finish_kernel); every other form leaves it 0
  kTimeouts = 6,    // waits inside a cooperative step end that gave up (sxmc_group_step_end_timeouts)
  kFillDone = 7,    // fused step: fill workgroups of this launch that have flushed
  kGate = 8,        // measurement build, the gated step: the finisher's "next proposal written"
  kTicketWords = 64,
};

}  // namespace sxstep
