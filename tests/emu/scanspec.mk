# TEST INFRASTRUCTURE ONLY: host builds of the step program with the key
# helper's speculative draw words (cotix_emu_scanspec.cpp = cotix_emu_keyl1.cpp
# + the draw ring's help policy), a build with M = 8 (the scan's round 0 past
# the kernel's M; with a small scene, lists shorter than M) and the stand-alone
# ASan/UBSan driver.
# make -C tests/emu -f scanspec.mk
CXX ?= g++
FLAGS = -DCOTIX_EMU_POISON -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_emu_scanspec.cpp cotix_emu_keyl1.cpp cotix_emu.cpp cotix_simt.h $(CS)/cotix_kernel.h $(CS)/cotix_plan.h \
	$(CS)/cotix_device.h $(CS)/cotix_scene.h $(CS)/cotix_grad.h $(CS)/cotix_body.h $(CS)/cotix_spec_hdrs.h

all: build/libcotix_emu_scanspec.so build/libcotix_emu_scanspec_m8.so build/scanspec_asan_driver

build/libcotix_emu_scanspec.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_emu_scanspec.cpp -o $@

build/libcotix_emu_scanspec_m8.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -DCOTIX_EMU_SCAN_M=8 -fPIC -shared cotix_emu_scanspec.cpp -o $@

build/scanspec_asan_driver: $(DEPS) scanspec_asan_driver.cpp keyl1_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_emu_scanspec.cpp scanspec_asan_driver.cpp -o $@
