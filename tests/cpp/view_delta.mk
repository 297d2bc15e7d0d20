# TEST binary: the drop-in's visible-delta shim (host/visible_delta.hpp) against the CPU reference-path system and a host loop over
# two ticks' isVisible bytes (view_delta.cpp; built and run by tests/test_gpu_view_delta.py). Links libgarden_vis.so (product) AND
# the oracle (checker) — tests only.
#   make -C tests/cpp -f view_delta.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/view_delta

$(OUT)/view_delta_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/view_delta_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/view_delta: view_delta.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/cpu_mesh_render_system.hpp \
                   $(OUT)/view_delta_oracle.o $(OUT)/view_delta_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) view_delta.cpp $(OUT)/view_delta_oracle.o $(OUT)/view_delta_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
