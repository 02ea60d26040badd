# tests/cpp/convolve_dropin: crlot::Convolver from a C++ caller (host code; g++).
# Links the product library only.  make -C tests/cpp -f convolve_dropin.mk
ROCM ?= /opt/rocm
CXXFLAGS := -std=c++17 -O2 -Wall -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I../../include
LIBS := -L../../crlot-dsp_amd -lcrlot_dsp -L$(ROCM)/lib -lamdhip64 \
        -Wl,-rpath,'$$ORIGIN/../../crlot-dsp_amd' -Wl,-rpath,$(ROCM)/lib
convolve_dropin: convolve_dropin.cpp ../../include/crlot_dsp.hpp ../../include/crlot_dsp.h
	g++ $(CXXFLAGS) -o $@ convolve_dropin.cpp $(LIBS)
