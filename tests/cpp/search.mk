# Builds the device::search_sorted test against include/simd_sort/radix_sort.hpp
# and ../../simd-radix-sort_amd/lib/libsrs_amd.so (hipcc for the HIP runtime
# headers): make -C tests/cpp -f search.mk
LIBDIR = $(abspath ../../simd-radix-sort_amd/lib)
.DEFAULT_GOAL := all
_build/test_search: test_search.cpp ../../include/simd_sort/radix_sort.hpp ../../include/srs_c_api.h
	@mkdir -p _build
	/opt/rocm/bin/hipcc -O2 -std=c++17 -I../../include -o $@ test_search.cpp \
	  -L$(LIBDIR) -lsrs_amd -Wl,-rpath,'$$ORIGIN/../../../simd-radix-sort_amd/lib'
all: _build/test_search
