# Builds the device::merge test against include/simd_sort/radix_sort.hpp
# and ../../simd-radix-sort_amd/lib/libsrs_amd.so (hipcc for the HIP runtime
# headers): make -C tests/cpp -f merge.mk
LIBDIR = $(abspath ../../simd-radix-sort_amd/lib)
.DEFAULT_GOAL := all
_build/test_merge: test_merge.cpp ../../include/simd_sort/radix_sort.hpp ../../include/srs_c_api.h
	@mkdir -p _build
	/opt/rocm/bin/hipcc -O2 -std=c++17 -I../../include -o $@ test_merge.cpp \
	  -L$(LIBDIR) -lsrs_amd -Wl,-rpath,'$$ORIGIN/../../../simd-radix-sort_amd/lib'
all: _build/test_merge
