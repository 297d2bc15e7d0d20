# TEST binary: the receiver-mask shim with pyramid slots (host/shadow_receivers.hpp, cullCascades): headless ticks — per cascade the
# main pass's receivers drawn into a mask whose pyramid lands in a slot of its own, then ONE cull of the main pass and the three
# cascades, each against its own pyramid — checked record for record against the one-at-a-time order (GpuShadowReceivers::cull), the
# main pass's depth pyramid read back before and after, and GpuSecondPhase of the main pass after the cascades against the host path
# (receivers_batched.cpp; run by tests/test_pyramid_slots_shim.py). Links libgarden_vis.so (product) AND the oracle (checker) — tests only.
#   make -C tests/cpp -f receivers_batched.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/receivers_batched

$(OUT)/receivers_batched_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/receivers_batched_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/receivers_batched: receivers_batched.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/gv_oracle.h \
                   $(OUT)/receivers_batched_oracle.o $(OUT)/receivers_batched_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) receivers_batched.cpp $(OUT)/receivers_batched_oracle.o $(OUT)/receivers_batched_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
