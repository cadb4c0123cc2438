# conv_plan_check: the convolution plan, its refusals and the plaintext sum's index lists of conv_plan.h (no HIP header) under AddressSanitizer / UBSan
# (no GPU, no library).
# make -C tests/host -f conv_plan.mk conv_plan_check
include Makefile
conv_plan_check: conv_plan_check.cpp $(PKG)/csrc/conv_plan.h
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ conv_plan_check.cpp
