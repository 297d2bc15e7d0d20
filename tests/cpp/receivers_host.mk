# TEST binary: the codes and the two-image rule of the receiver-mask calls (receivers_host_test.cpp; run by
# tests/test_receivers_host.py) against the library as it is built for the device. Links libgarden_vis.so only: no oracle, no sanitizer.
#   make -C tests/cpp -f receivers_host.mk
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -pthread

all: $(OUT)/receivers_host_test

$(OUT)/receivers_host_test: receivers_host_test.cpp $(ROOT)/include/garden_vis.h $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) receivers_host_test.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
