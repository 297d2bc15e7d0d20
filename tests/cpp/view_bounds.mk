# TEST binary: the drop-in's view-bounds shim (host/view_bounds.hpp) against a host loop over the delivered list
# (view_bounds.cpp; built and run by tests/test_gpu_view_bounds.py). Links libgarden_vis.so only: no oracle.
#   make -C tests/cpp -f view_bounds.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include

all: $(OUT)/view_bounds

$(OUT)/view_bounds: view_bounds.cpp $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) view_bounds.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,$(abspath $(ROOT)/garden_amd/lib) -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
