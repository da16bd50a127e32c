# The C++ programs of the CORRELATED PROPOSAL's tests (make -C tests/cpp -f proposal.mk); the Makefile and mixed.mk
# beside it keep the drivers that were there before.
CXX ?= g++
ROOT := ../..
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread

all: proposal_factor_host proposal_factor_host_asan test_proposal_plan test_proposal_plan_asan proposal_walk proposal_mixed_walk

# no device, no library: the re-tuning (sxmc_amd/csrc/proposal_factor.h, behind sxmc_proposal_factor) on case files,
# plain and under ASan + UBSan.  -ffp-contract=off as the library is built: every operation rounds on its own.
PROPOSAL_FACTOR_DEPS = proposal_factor_host.cpp $(ROOT)/sxmc_amd/csrc/proposal_factor.h
proposal_factor_host: $(PROPOSAL_FACTOR_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -o $@ proposal_factor_host.cpp

proposal_factor_host_asan: $(PROPOSAL_FACTOR_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ proposal_factor_host.cpp

# no device needed: the correlated proposal in the walk's plan (walk_plan.h), plain and under ASan + UBSan
PROPOSAL_PLAN_DEPS = test_proposal_plan.cpp mini_test.h $(ROOT)/sxmc_amd/include/sxmc/walk_plan.h
test_proposal_plan: $(PROPOSAL_PLAN_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ test_proposal_plan.cpp

test_proposal_plan_asan: $(PROPOSAL_PLAN_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ test_proposal_plan.cpp

# walks of sxmc::MCMC over the small fit with the correlated proposal in every sequential form, for
# tests/test_gpu_proposal_cpp.py
proposal_walk: proposal_walk.cpp small_fit.h $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ proposal_walk.cpp $(LDFLAGS)

# walks over a mixed histogram + kernel-density fit with the correlated proposal, for tests/test_gpu_proposal_mixed.py
proposal_mixed_walk: proposal_mixed_walk.cpp $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ proposal_mixed_walk.cpp $(LDFLAGS)

clean:
	rm -f proposal_factor_host proposal_factor_host_asan test_proposal_plan test_proposal_plan_asan proposal_walk proposal_mixed_walk

.PHONY: all clean
