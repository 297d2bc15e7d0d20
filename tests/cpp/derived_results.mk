# TEST binary: the tables of the derived results (derived_results_test.cpp; run by tests/test_derived_results.py) against the
# library as it is built for the device. Links libgarden_vis.so only: no oracle, no sanitizer.
#   make -C tests/cpp -f derived_results.mk
CXX ?= g++
ROOT = ../..
OUT = build
CXXFLAGS = -O2 -std=c++17 -Wall -Wextra -pthread

all: $(OUT)/derived_results_test

$(OUT)/derived_results_test: derived_results_test.cpp $(ROOT)/include/garden_vis.h $(ROOT)/garden_amd/lib/libgarden_vis.so
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) derived_results_test.cpp -o $@ -L$(ROOT)/garden_amd/lib -lgarden_vis \
	    -Wl,-rpath,'$$ORIGIN/../../../garden_amd/lib' -Wl,-rpath,/opt/rocm/lib -L/opt/rocm/lib -lamdhip64 -lm -lpthread

.PHONY: all
