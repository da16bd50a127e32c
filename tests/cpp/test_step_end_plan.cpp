// test_step_end_plan.cpp -- the pure parts of the end of a Metropolis step (sxmc_amd/csrc/step_end_plan.h: the blocks of
// the event sum, the chunks of the clearing, the kernels' LDS size, the words of the ticket block) checked without a
// device or the library.  Stand-alone, so that tests/test_step_end_plan_cpu.py can also build and run it under ASan +
// UBSan.  Exit status 0 and "test_step_end_plan: ok" when every check holds.
#include <cstdio>

#include "../../sxmc_amd/csrc/step_end_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("test_step_end_plan: line %d: %s\n", __LINE__, #cond);   \
      failures++;                                                          \
    }                                                                      \
  } while (0)

using namespace sxstep;

int main() {
  // ---- the event sum: blocks of 128 rows, at least one, at most 1024 (the partial sums' buffer)
  {
    const struct { unsigned long long ne; int blocks; } pinned[] = {
        {0, 1}, {1, 1}, {128, 1}, {129, 2}, {131072, 1024}, {131073, 1024},
    };
    for (const auto& c : pinned) CHECK(step_sum_blocks(c.ne) == c.blocks);
    // every row has a block while the cap is not reached; the one-workgroup form's rows make at most two
    for (unsigned long long ne = 1; ne <= 131072; ne += 37) {
      const unsigned long long b = (unsigned long long)step_sum_blocks(ne);
      CHECK(b * kStepSumRows >= ne && (b - 1) * kStepSumRows < ne);
    }
    CHECK(step_sum_blocks(kTailMaxLookups) <= 2);
  }

  // ---- the clearing: one 16-byte store per lane, chunk and round; at least one chunk (it clears the n & 3 tail), at
  // most 1024 unless the caller says otherwise
  {
    const int most = 4 * 128 * 1024;
    const struct { int max_bins, block, chunks; } pinned[] = {
        {0, 128, 1},    {3, 128, 1},    {4, 128, 1},    {511, 128, 1},       {512, 128, 1},
        {513, 128, 1},  {516, 128, 2},  {most, 128, 1024}, {most + 1, 128, 1024}, {most + 4, 128, 1024},
        {0, 256, 1},    {3, 256, 1},    {4, 256, 1},    {511, 256, 1},       {512, 256, 1},
        {513, 256, 1},  {1028, 256, 2}, {most, 256, 512},  {most + 1, 256, 512},
    };
    for (const auto& c : pinned) CHECK(zero_blocks(c.max_bins, c.block) == c.chunks);
    CHECK(zero_blocks(1 << 23, 256) == 1024 && zero_blocks(1 << 23, 256, 2048) == 2048);   // (zero_kernel's cap)
    // below the cap the chunks' lanes cover every whole 16-byte store in one round, and one chunk fewer would not
    for (int block : {128, 256}) {
      for (int bins = 0; bins < 4 * block * 1024; bins += 4099) {
        const long long chunks = zero_blocks(bins, block);
        CHECK(chunks * block >= bins / 4 && (chunks == 1 || (chunks - 1) * block < bins / 4));
      }
    }
  }

  // ---- LDS of the kernels over eval_nll_block_part: 16 wave sums + the members' records in whole passes of 16
  for (size_t nsig : {(size_t)0, (size_t)1, (size_t)16, (size_t)17, (size_t)1024}) {
    CHECK(step_end_lds_bytes(nsig) == 16 * sizeof(double) + ((nsig + 15) / 16 * 16) * 48);
  }
  CHECK(step_end_lds_bytes(0) == 128 && step_end_lds_bytes(1) == 896 && step_end_lds_bytes(16) == 896);
  CHECK(step_end_lds_bytes(17) == 1664 && step_end_lds_bytes(1024) == 49280);

  // ---- the ticket block's words: distinct, inside the block
  {
    const unsigned words[] = {kTicket, kTimeouts, kFillDone, kGate};
    for (size_t i = 0; i < 4; i++) {
      CHECK(words[i] < kTicketWords);
      for (size_t j = i + 1; j < 4; j++) CHECK(words[i] != words[j]);
    }
    CHECK(kTicket == 0);   // (zero_kernel and finish_zero_kernel are handed the block's address as the ticket's)
    CHECK(kCoopMaxWorkers == (int)kStepSumRows);   // one lane of the finisher per slot
  }

  if (failures == 0) std::printf("test_step_end_plan: ok\n");
  return failures == 0 ? 0 : 1;
}
