# TEST INFRASTRUCTURE ONLY: the host checker of cotix_raycast_backward
# (cotix_raygrad_host.cpp: a loop over envs, rays and output slots around the
# functions of cotix_raycast_grad.h) and its stand-alone ASan/UBSan driver.
# make -C tests/emu -f raygrad.mk
CXX ?= g++
FLAGS = -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_raygrad_host.cpp $(CS)/cotix_raycast_grad.h $(CS)/cotix_raycast.h $(CS)/cotix_raster.h \
	$(CS)/cotix_body.h $(CS)/cotix_device.h ../../include/cotix_amd.h

all: build/libcotix_raygrad_host.so build/raygrad_asan_driver

build/libcotix_raygrad_host.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_raygrad_host.cpp -o $@

build/raygrad_asan_driver: $(DEPS) raygrad_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_raygrad_host.cpp raygrad_asan_driver.cpp -o $@
