# test_regression_data: the reference's Test_Regression driver from a data file to theta / det modulo p, on the C++ mirror's slot layer.
# Same compiler, flags, headers and link line as the harness programs of ./Makefile;  make -C tests/host -f regression_data.mk test_regression_data
include Makefile
test_regression_data: test_regression_data.cpp $(HDRS) $(LIBDIR)/libfhesi_hip.so
	$(CXX) $(CXXFLAGS) -o $@ $< $(LINK)
