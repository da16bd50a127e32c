# The C++ programs of the MIXED walk's tests (make -C tests/cpp -f mixed.mk): same compiler, flags and library as the
# Makefile beside it, which keeps the drivers that were there before.
CXX ?= g++
ROOT := ../..
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread

all: test_mixed_plan test_mixed_plan_asan mixed_walk

# no device needed: the form of a MIXED walk's steps (walk_plan.h), the column table of sxmc_group_set_columns
# (sxmc_plan.h) and the null-handle answers of the mixed entry points (the library is linked, no device call is made);
# plain and under ASan + UBSan
MIXED_PLAN_DEPS = test_mixed_plan.cpp mini_test.h $(ROOT)/sxmc_amd/include/sxmc/walk_plan.h $(ROOT)/sxmc_amd/csrc/sxmc_plan.h \
                  $(ROOT)/sxmc_amd/csrc/sxmc_device_types.h $(ROOT)/include/sxmc_hip.h
test_mixed_plan: $(MIXED_PLAN_DEPS)
	$(CXX) $(CXXFLAGS) -o $@ test_mixed_plan.cpp $(LDFLAGS)

test_mixed_plan_asan: $(MIXED_PLAN_DEPS)
	$(CXX) $(CXXFLAGS) -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ test_mixed_plan.cpp $(LDFLAGS)

# walks of sxmc::MCMC over mixed histogram + kernel-density fits in every form, and their timing (--bench), for
# tests/test_gpu_mixed_walk.py and the README's "Mixed walks"
mixed_walk: mixed_walk.cpp $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ mixed_walk.cpp $(LDFLAGS)

clean:
	rm -f test_mixed_plan test_mixed_plan_asan mixed_walk

.PHONY: all clean
