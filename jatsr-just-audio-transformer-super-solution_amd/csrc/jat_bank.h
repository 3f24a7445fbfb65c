// The bank handle of latent retrieval (include/jat_hip.h): created and filled by jat_retrieval.cpp, clustered by
// jat_retrieval_km.cpp.
#pragma once
#include <stdint.h>

struct jat_bank {
  int channels = 0, capacity = 0, size = 0;
  bool paired = false;
  uint16_t *keys = nullptr, *values = nullptr;   // [capacity, channels] fp16; values == keys unless paired
  float* norms = nullptr;                        // |key row|^2, capacity rounded up to whole key tiles
};
