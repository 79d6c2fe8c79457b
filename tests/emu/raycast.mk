# TEST INFRASTRUCTURE ONLY: the host checker of cotix_raycast
# (cotix_raycast_host.cpp: a loop over envs and rays around the functions of
# cotix_raycast.h) and its stand-alone ASan/UBSan driver.
# make -C tests/emu -f raycast.mk
CXX ?= g++
FLAGS = -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_raycast_host.cpp $(CS)/cotix_raycast.h $(CS)/cotix_raster.h $(CS)/cotix_body.h $(CS)/cotix_device.h \
	../../include/cotix_amd.h

all: build/libcotix_raycast_host.so build/raycast_asan_driver

build/libcotix_raycast_host.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_raycast_host.cpp -o $@

build/raycast_asan_driver: $(DEPS) raycast_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_raycast_host.cpp raycast_asan_driver.cpp -o $@
