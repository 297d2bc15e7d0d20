# TEST binary: the drop-in's occluder shim (host/occluders.hpp): a headless frame — cull, draw occluders, build, second phase —
# against the CPU reference-path system fed the fetched image (occluders.cpp; run by tests/test_occluders_host.py). Links libgarden_vis.so (product) AND
# the oracle (checker) — tests only.
#   make -C tests/cpp -f occluders.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/occluders

$(OUT)/occluders_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/occluders_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/occluders: occluders.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/cpu_mesh_render_system.hpp \
                   $(OUT)/occluders_oracle.o $(OUT)/occluders_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) occluders.cpp $(OUT)/occluders_oracle.o $(OUT)/occluders_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
