# TEST binary: the codes, lifetimes and the image-taking rule of the pyramid slots (pyramid_slots_host_test.cpp; run by
# tests/test_pyramid_slots_host.py) against the library as it is built for the device. Links libgarden_vis.so only: no oracle, no sanitizer.
#   make -C tests/cpp -f pyramid_slots_host.mk
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -pthread

all: $(OUT)/pyramid_slots_host_test

$(OUT)/pyramid_slots_host_test: pyramid_slots_host_test.cpp $(ROOT)/include/garden_vis.h $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) pyramid_slots_host_test.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
