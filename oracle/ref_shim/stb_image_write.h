/*
 * stb_image_write.h -- stand-in for the one call write_mat (main.cu:13-35) makes into the PNG writer the reference vendors.
 * TEST INFRASTRUCTURE, used only by the copy of write_mat that oracle/ref_build.py cuts out of main.cu.
 *
 * Nothing is encoded: the w * h * comp bytes write_mat hands over -- the normalised 8-bit image -- go as they are to the file
 * the driver has opened (ref_capture_file, cuda_runtime.h).  Returns 1 like the writer it stands for, 0 on a short write.
 */
#pragma once

int stbi_write_png(const char* filename, int w, int h, int comp, const void* data, int stride_in_bytes);
