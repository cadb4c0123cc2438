# poly_plan_check: the Paterson-Stockmeyer planner and schedule of poly_plan.h (no HIP header) under AddressSanitizer / UBSan (no GPU, no library).
# make -C tests/host -f poly_plan.mk poly_plan_check
include Makefile
poly_plan_check: poly_plan_check.cpp $(PKG)/csrc/poly_plan.h
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ poly_plan_check.cpp
