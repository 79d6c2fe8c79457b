# TEST INFRASTRUCTURE ONLY: host builds of the backward with the shape
# geometry's gradient (cotix_emu_gradg.cpp = cotix_emu.cpp + the level-2 wave
# programs): the plain library, phase G's tile form on every scene
# (-DCOTIX_NO_GREGS), and the stand-alone ASan/UBSan driver.
# make -C tests/emu -f gradg.mk
CXX ?= g++
FLAGS = -DCOTIX_EMU_POISON -std=c++17 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unknown-pragmas
CS = ../../parallax_amd/csrc
DEPS = cotix_emu_gradg.cpp cotix_emu.cpp cotix_simt.h $(CS)/cotix_kernel.h $(CS)/cotix_plan.h $(CS)/cotix_device.h $(CS)/cotix_scene.h \
	$(CS)/cotix_grad.h $(CS)/cotix_body.h $(CS)/cotix_spec_hdrs.h

all: build/libcotix_emu_gradg.so build/libcotix_emu_gradg_nogregs.so build/gradg_asan_driver

build/libcotix_emu_gradg.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -fPIC -shared cotix_emu_gradg.cpp -o $@

build/libcotix_emu_gradg_nogregs.so: $(DEPS)
	@mkdir -p build
	$(CXX) -O2 $(FLAGS) -DCOTIX_NO_GREGS -fPIC -shared cotix_emu_gradg.cpp -o $@

build/gradg_asan_driver: $(DEPS) gradg_asan_driver.cpp
	@mkdir -p build
	$(CXX) -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all $(FLAGS) \
		cotix_emu_gradg.cpp gradg_asan_driver.cpp -o $@
