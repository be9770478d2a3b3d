# TEST INFRASTRUCTURE: the host-only arithmetic of the token server stat log (sentinel_amd/csrc/serverlog_rules.h) on
# the CPU, under the address and undefined-behaviour sanitizers (its own main, no GPU, no HIP; the sanitizer runtimes
# linked statically). Built in-tree by __graft_entry__.build(); run by tests/test_serverlog_host.py.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
OUT   := $(ROOT)/build/tests

all: $(OUT)/test_serverlog_host

$(OUT)/test_serverlog_host: $(HERE)test_serverlog_host.cpp $(ROOT)/sentinel_amd/csrc/serverlog_rules.h \
                            $(ROOT)/include/sentinel_gpu.h
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
	    -static-libubsan -o $@ $<

.PHONY: all
