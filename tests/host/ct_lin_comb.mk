# ct_lin_comb_check: the scalar linear combination of ct_wide.h behind the term lists of poly_plan.h (neither includes a HIP header) under AddressSanitizer /
# UBSan (no GPU, no library).  make -C tests/host -f ct_lin_comb.mk ct_lin_comb_check
include Makefile
ct_lin_comb_check: ct_lin_comb_check.cpp $(PKG)/csrc/ct_wide.h $(PKG)/csrc/poly_plan.h
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ ct_lin_comb_check.cpp
