# lattice_plan_check: the plans of a strided / dilated convolution and of a sum pooling of lattice_plan.h (no HIP header) and their refusals under
# AddressSanitizer / UBSan (no GPU, no library).
# make -C tests/host -f lattice_plan.mk lattice_plan_check
include Makefile
lattice_plan_check: lattice_plan_check.cpp $(PKG)/csrc/lattice_plan.h $(PKG)/csrc/conv_plan.h
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ lattice_plan_check.cpp
