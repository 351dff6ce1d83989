/* Stand-in for NVIDIA's NVTX header: the reference includes it but calls nothing from it. */
