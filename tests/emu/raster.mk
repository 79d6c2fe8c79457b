# TEST INFRASTRUCTURE ONLY: the host checker of cotix_rasterize
# (cotix_raster_host.cpp: a loop over envs and pixels around the functions of
# cotix_raster.h) and its stand-alone ASan/UBSan driver.
# make -C tests/emu -f raster.mk
CXX ?= g++
FLAGS = -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_raster_host.cpp $(CS)/cotix_raster.h $(CS)/cotix_body.h $(CS)/cotix_device.h ../../include/cotix_amd.h

all: build/libcotix_raster_host.so build/raster_asan_driver

build/libcotix_raster_host.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_raster_host.cpp -o $@

build/raster_asan_driver: $(DEPS) raster_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_raster_host.cpp raster_asan_driver.cpp -o $@
