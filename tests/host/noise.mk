# test_noise: FHESISecKey::NoiseBudget / NoiseBudgetBatch on the C++ mirror, recorded, at once and from toPoly in ZZ.
# Same compiler, flags, headers and link line as the harness programs of ./Makefile;  make -C tests/host -f noise.mk test_noise
include Makefile
test_noise: test_noise.cpp $(HDRS) $(LIBDIR)/libfhesi_hip.so
	$(CXX) $(CXXFLAGS) -o $@ $< $(LINK)
