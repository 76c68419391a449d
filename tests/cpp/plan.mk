# Builds the planner's sanitizer check: csrc/srs_plan.hip and plan_check.cpp
# for the host only, with AddressSanitizer and UBSan (no device code, no
# library): make -C tests/cpp -f plan.mk
CSRC = ../../simd-radix-sort_amd/csrc
SAN = -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined
.DEFAULT_GOAL := all
_build/plan_check: plan_check.cpp $(CSRC)/srs_plan.hip $(CSRC)/srs_plan.h $(CSRC)/srs_common.h
	@mkdir -p _build
	/opt/rocm/bin/hipcc -O1 -g -std=c++17 -Wall --offload-host-only $(SAN) -I$(CSRC) -o $@ \
	  -x hip plan_check.cpp $(CSRC)/srs_plan.hip
all: _build/plan_check
