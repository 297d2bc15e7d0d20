# TEST binary: the cluster-command shim (host/cluster_commands.hpp behind GpuDrawCommands): headless ticks with a main pass and three
# cascades, a moving camera and LODs, every cluster command against a host path that fetches the records and calls the oracle
# (cluster_commands.cpp; run by tests/test_gpu_clusters.py). Links libgarden_vis.so (product) AND the oracle (checker) — tests only.
#   make -C tests/cpp -f cluster_commands.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -Wno-unused-function -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/cluster_commands

$(OUT)/cluster_commands_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/cluster_commands_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/cluster_commands: cluster_commands.cpp ../cluster_twin.h ../lod_twin.h $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/gv_oracle.h \
                   $(OUT)/cluster_commands_oracle.o $(OUT)/cluster_commands_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) cluster_commands.cpp $(OUT)/cluster_commands_oracle.o $(OUT)/cluster_commands_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
