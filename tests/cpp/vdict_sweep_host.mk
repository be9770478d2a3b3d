# TEST INFRASTRUCTURE: the host-side rules of the value dictionary's sweep (sentinel_amd/csrc/vdict_sweep.h) on the CPU,
# under the address and undefined-behaviour sanitizers (its own main, no GPU, no HIP; the sanitizer runtimes linked
# statically). Built in-tree by __graft_entry__.build(); run by tests/test_vdict_sweep_host.py.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
OUT   := $(ROOT)/build/tests

all: $(OUT)/test_vdict_sweep_host

$(OUT)/test_vdict_sweep_host: $(HERE)test_vdict_sweep_host.cpp $(ROOT)/sentinel_amd/csrc/vdict_sweep.h
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
	    -static-libubsan -o $@ $<

.PHONY: all
