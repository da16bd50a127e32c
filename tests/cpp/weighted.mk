# The C++ programs of the WEIGHTED EVENTS' tests (make -C tests/cpp -f weighted.mk); the Makefile, mixed.mk and proposal.mk
# beside it keep the drivers that were there before.
CXX ?= g++
ROOT := ../..

CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread

all: weighted_classes_host weighted_classes_host_asan test_weighted_plan test_weighted_plan_asan weighted_walk

# no device, no library: the classes' weight sums (sxmc_amd/csrc/sxmc_plan.h, behind sxmc_group_set_event_weights) on
# case files, plain and under ASan + UBSan.  -ffp-contract=off as the library is built: every operation rounds on its own.
WEIGHTED_CLASSES_DEPS = weighted_classes_host.cpp $(ROOT)/sxmc_amd/csrc/sxmc_plan.h $(ROOT)/sxmc_amd/csrc/sxmc_device_types.h
weighted_classes_host: $(WEIGHTED_CLASSES_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -I$(ROOT)/sxmc_amd/csrc -o $@ weighted_classes_host.cpp

weighted_classes_host_asan: $(WEIGHTED_CLASSES_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$(ROOT)/sxmc_amd/csrc -o $@ weighted_classes_host.cpp

# no device needed: weighted events in the walk's plan (walk_plan.h), plain and under ASan + UBSan
WEIGHTED_PLAN_DEPS = test_weighted_plan.cpp mini_test.h $(ROOT)/sxmc_amd/include/sxmc/walk_plan.h
test_weighted_plan: $(WEIGHTED_PLAN_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ test_weighted_plan.cpp

test_weighted_plan_asan: $(WEIGHTED_PLAN_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ test_weighted_plan.cpp

# walks of sxmc::MCMC over the small fit with weighted events in every sequential form, for tests/test_gpu_weighted_walk.py
weighted_walk: weighted_walk.cpp small_fit.h $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ weighted_walk.cpp $(LDFLAGS)

clean:
	rm -f weighted_classes_host weighted_classes_host_asan test_weighted_plan test_weighted_plan_asan weighted_walk

.PHONY: all clean
