# TEST binary: the drop-in's second-phase shim (host/second_phase.hpp) against a host loop over the two fetched lists
# (second_phase.cpp; run by tests/test_gpu_second_phase.py). Links libgarden_vis.so only: no oracle.
#   make -C tests/cpp -f second_phase.mk
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include

all: $(OUT)/second_phase

$(OUT)/second_phase: second_phase.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) second_phase.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
