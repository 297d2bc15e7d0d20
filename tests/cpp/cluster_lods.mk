# TEST binary: the level-of-detail form of the cluster cull through the shim (GpuClusterCommands::setClusterLods / setLodViews of host/cluster_commands.hpp): headless
# ticks with a moving camera and one cascade, every command of gv_pool_cull_cluster_lods against a host path over the oracle and the
# twin of the LOD rule (cluster_lods.cpp; run by tests/test_gpu_cluster_lods_shim.py). Links libgarden_vis.so (product) AND the oracle
# (checker) — tests only.
#   make -C tests/cpp -f cluster_lods.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -Wno-unused-function -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
ORACLE_FLAGS = -O2 -march=haswell -ffp-contract=off -fno-fast-math -std=c11 -pthread

all: $(OUT)/cluster_lods

$(OUT)/cluster_lods_oracle.o: $(ROOT)/oracle/gv_oracle.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle.c -o $@
$(OUT)/cluster_lods_oracle_avx2.o: $(ROOT)/oracle/gv_oracle_avx2.c $(ROOT)/oracle/gv_oracle.h
	@mkdir -p $(OUT)
	gcc $(ORACLE_FLAGS) -c $(ROOT)/oracle/gv_oracle_avx2.c -o $@

$(OUT)/cluster_lods: cluster_lods.cpp ../cluster_twin.h ../cluster_runs_twin.h ../cluster_cone_twin.h ../cluster_lod_twin.h $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/oracle/gv_oracle.h \
                   $(OUT)/cluster_lods_oracle.o $(OUT)/cluster_lods_oracle_avx2.o $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) cluster_lods.cpp $(OUT)/cluster_lods_oracle.o $(OUT)/cluster_lods_oracle_avx2.o -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
