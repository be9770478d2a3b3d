# TEST INFRASTRUCTURE: the gateway API definitions' host side and the matcher host and device share
# (sentinel_amd/csrc/gateway_api.h: validity, classification, the Ant matcher, the lookup tables, the verdict ids) on
# the CPU, under the address and undefined-behaviour sanitizers (its own main, no GPU, no HIP; the sanitizer runtimes
# linked statically). Built in-tree by __graft_entry__.build(); run by tests/test_gateway_api_host.py.
HERE  := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
ROOT  := $(HERE)../..
OUT   := $(ROOT)/build/tests

all: $(OUT)/test_gateway_api_host

$(OUT)/test_gateway_api_host: $(HERE)test_gateway_api_host.cpp $(ROOT)/sentinel_amd/csrc/gateway_api.h \
                              $(ROOT)/sentinel_amd/csrc/gateway_rules.h $(ROOT)/include/sentinel_gpu.h
	@mkdir -p $(OUT)
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan \
	    -static-libubsan -o $@ $<

.PHONY: all
