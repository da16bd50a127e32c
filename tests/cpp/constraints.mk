# The C++ programs of the tests of CORRELATED GAUSSIAN CONSTRAINTS (make -C tests/cpp -f constraints.mk); the other
# makefiles beside it keep the drivers that were there before.
CXX ?= g++
ROOT := ../..

CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread
HEADERS = $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h

all: constraint_whitening_host constraint_whitening_host_asan test_constraint_plan test_constraint_plan_asan constraint_config_dump constraint_walk

# no device, no library: the validation and the whitening (sxmc_amd/csrc/constraint_whitening.h, behind
# sxmc_constraint_whitening) on case files, plain and under ASan + UBSan.  -ffp-contract=off as the library is built: every
# operation rounds on its own.
WHITENING_DEPS = constraint_whitening_host.cpp $(ROOT)/sxmc_amd/csrc/constraint_whitening.h
constraint_whitening_host: $(WHITENING_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -o $@ constraint_whitening_host.cpp

constraint_whitening_host_asan: $(WHITENING_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ constraint_whitening_host.cpp

# no device needed: correlated constraints in the walk's plan (walk_plan.h), plain and under ASan + UBSan
CONSTRAINT_PLAN_DEPS = test_constraint_plan.cpp mini_test.h $(ROOT)/sxmc_amd/include/sxmc/walk_plan.h
test_constraint_plan: $(CONSTRAINT_PLAN_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ test_constraint_plan.cpp

test_constraint_plan_asan: $(CONSTRAINT_PLAN_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ test_constraint_plan.cpp

# no device call: the fit's "constraint_correlations" as sxmc::load_config reads them, for
# tests/test_constraint_config_cpu.py
constraint_config_dump: constraint_config_dump.cpp $(HEADERS)
	$(CXX) $(CXXFLAGS) -o $@ constraint_config_dump.cpp $(LDFLAGS)

# walks of sxmc::MCMC with correlated constraints in every sequential form, and the bench, for
# tests/test_gpu_constraint_cpp.py
constraint_walk: constraint_walk.cpp small_fit.h $(HEADERS)
	$(CXX) $(CXXFLAGS) -o $@ constraint_walk.cpp $(LDFLAGS)

clean:
	rm -f constraint_whitening_host constraint_whitening_host_asan test_constraint_plan test_constraint_plan_asan constraint_config_dump constraint_walk

.PHONY: all clean
