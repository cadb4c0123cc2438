# test_regression_pow2: the data-file regression driver on a power-of-two ring (two-row slot space), on the C++ mirror.
# Same compiler, flags, headers and link line as the harness programs of ./Makefile;  make -C tests/host -f regression_pow2.mk test_regression_pow2
include Makefile
test_regression_pow2: test_regression_pow2.cpp $(HDRS) $(LIBDIR)/libfhesi_hip.so
	$(CXX) $(CXXFLAGS) -o $@ $< $(LINK)
