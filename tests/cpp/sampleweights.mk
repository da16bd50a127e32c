# The C++ programs of the WEIGHTED MONTE CARLO SAMPLES' tests (make -C tests/cpp -f sampleweights.mk); the other makefiles
# beside it keep the drivers that were there before.
CXX ?= g++
ROOT := ../..

CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-unused-parameter -I$(ROOT)/sxmc_amd/include/spelling -I$(ROOT)/include -pthread
LDFLAGS = -L$(ROOT)/sxmc_amd/csrc -lsxmc_hip -Wl,-rpath,'$$ORIGIN/../../sxmc_amd/csrc' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath-link,/opt/rocm/lib -pthread

all: sample_weights_host sample_weights_host_asan sample_weights_walk

# walks of sxmc::MCMC over signals with sample multiplicities in every sequential form, for
# tests/test_gpu_weighted_fill_walk.py
sample_weights_walk: sample_weights_walk.cpp small_fit.h $(wildcard $(ROOT)/sxmc_amd/include/sxmc/*.h) $(wildcard $(ROOT)/sxmc_amd/include/spelling/*/*.h) $(ROOT)/include/sxmc_hip.h
	$(CXX) $(CXXFLAGS) -o $@ sample_weights_walk.cpp $(LDFLAGS)

# no device, no library: the quantiser (sxmc_amd/csrc/sample_multiplicities.h, behind sxmc_sample_multiplicities) on case
# files, plain and under ASan + UBSan
SAMPLE_WEIGHTS_DEPS = sample_weights_host.cpp $(ROOT)/sxmc_amd/csrc/sample_multiplicities.h
sample_weights_host: $(SAMPLE_WEIGHTS_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -ffp-contract=off -o $@ sample_weights_host.cpp

sample_weights_host_asan: $(SAMPLE_WEIGHTS_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -o $@ sample_weights_host.cpp

clean:
	rm -f sample_weights_host sample_weights_host_asan sample_weights_walk

.PHONY: all clean
