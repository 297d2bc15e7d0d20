# TEST binary: the drop-in's receiver-mask shim (host/shadow_receivers.hpp): headless ticks — the main pass and three cascades culled,
# per cascade the main pass's receivers drawn into a mask, its pyramid built, the cascade culled again against it — checked list by
# list against the host path (the oracle's cull, fed the fetched mask) (receivers.cpp; run by tests/test_receivers_host.py). Links
# libgarden_vis.so (product) AND the oracle (checker) — tests only.
#   make -C tests/cpp -f receivers.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/receivers

$(OUT)/receivers_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/receivers_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/receivers: receivers.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/gv_oracle.h \
                   $(OUT)/receivers_oracle.o $(OUT)/receivers_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) receivers.cpp $(OUT)/receivers_oracle.o $(OUT)/receivers_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
