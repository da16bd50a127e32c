# The C++ programs of the tests of WEIGHTED MONTE CARLO SAMPLES IN pdfz::EvalKernel (make -C tests/cpp -f kdeweights.mk);
# the other makefiles beside it keep the drivers that were there before.
CXX ?= g++
ROOT := ../..

CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread

all: kde_weights_host kde_weights_host_asan kde_weights_walk

# a small mixed fit whose kernel-density signal carries multiplicities, in three forms of sxmc::MCMC's walk, and
# build_pdfz's refusals, for tests/test_gpu_kde_weighted_walk.py
kde_weights_walk: kde_weights_walk.cpp small_fit.h $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ kde_weights_walk.cpp $(LDFLAGS)

# no device, no library: the bandwidth law (sxmc_amd/csrc/kde_weights.h, behind sxmc_kde_create_weighted and
# sxmc_kde_weighted_bandwidths) on case files, plain and under ASan + UBSan
KDE_WEIGHTS_DEPS = kde_weights_host.cpp $(ROOT)/sxmc_amd/csrc/kde_weights.h $(ROOT)/sxmc_amd/csrc/kde_plan.h
kde_weights_host: $(KDE_WEIGHTS_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -o $@ kde_weights_host.cpp

kde_weights_host_asan: $(KDE_WEIGHTS_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ kde_weights_host.cpp

clean:
	rm -f kde_weights_host kde_weights_host_asan kde_weights_walk

.PHONY: all clean
