# TEST binary: the drop-in's motion-history shim (host/motion_history.hpp): five headless ticks — a moving camera, movers, a cut, a
# forgotten range — with GpuInstanceWriter::write and GpuMotionHistory::write into one {mvp, prevMvp, hasHistory} array, checked byte
# for byte against the draw loop restated through the twins (motion_history.cpp; run by tests/test_gpu_previous.py). Links
# libgarden_vis.so only.
#   make -C tests/cpp -f motion_history.mk [OUT=dir]
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -Wno-invalid-offsetof -fno-strict-aliasing -march=haswell -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include

all: $(OUT)/motion_history

$(OUT)/motion_history: motion_history.cpp ../previous_twin.h ../instance_twin.h $(ROOT)/garden_amd/csrc/host/*.hpp $(ROOT)/include/garden_vis.h \
                       $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) motion_history.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
