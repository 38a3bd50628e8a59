// qa_radiance.h — what qa_radiance.hip offers the other units of libqaray_hip.so.  Not part of the C ABI.
#pragma once

struct qa_ctx;

// Frees the staging buffer of the context's host-form radiance queries, if it made one (qa_ctx_destroy)
void FreeRadianceStage(qa_ctx *c);
