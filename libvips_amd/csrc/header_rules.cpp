// The reference's rules about an image's header (iofuncs/header.c) and the small conversions every op family needs
// of them, once: what a tag says about the bands, the alpha range and whether it can be true of the image; a constant
// as an element of a band format; the non-complex check.
#include "internal.h"

#include <climits>
#include <cstring>

using namespace vh;

// vips_interpretation_bands, iofuncs/header.c:218-249 (the reference's numbers: a .v file can carry a tag that
// vips_hip.h has no name for), for vips_image_hasalpha, image.c:3113, and the guess below
int vh::interpretation_bands(int interpretation)
{
	switch (interpretation) {
	case 1:  // B_W
	case 26: // GREY16
		return 1;
	case 17: // RGB
	case 18: // CMC
	case 19: // LCH
	case 21: // LABS
	case 22: // sRGB
	case 23: // YXY
	case 12: // XYZ
	case 13: // LAB
	case 25: // RGB16
	case 28: // scRGB
	case 29: // HSV
	case 30: // OKLAB
	case 31: // OKLCH
		return 3;
	case 15: // CMYK
		return 4;
	default:
		return 0;
	}
}

// vips_interpretation_max_alpha, iofuncs/header.c:194-206
double vh::interpretation_max_alpha(int interpretation)
{
	switch (interpretation) {
	case VIPS_HIP_INTERPRETATION_GREY16:
	case VIPS_HIP_INTERPRETATION_RGB16:
		return 65535.0;
	case VIPS_HIP_INTERPRETATION_scRGB:
		return 1.0;
	default:
		return 255.0;
	}
}

// vips_image_guess_interpretation, iofuncs/header.c:589-759, for uncoded images: the tag, unless it cannot be true of
// such an image -- then vips_image_default_interpretation's answer for the format and the bands
int vh::guess_interpretation(int type, int width, int height, int bands, int format)
{
	bool sane = bands >= interpretation_bands(type);
	const bool is8 = format == VIPS_HIP_FORMAT_UCHAR || format == VIPS_HIP_FORMAT_CHAR;
	const bool isuint = format == VIPS_HIP_FORMAT_UCHAR || format == VIPS_HIP_FORMAT_USHORT || format == VIPS_HIP_FORMAT_UINT;
	const bool isfloat = format == VIPS_HIP_FORMAT_FLOAT || format == VIPS_HIP_FORMAT_DOUBLE;
	switch (type) {
	case -1: // ERROR
	case VIPS_HIP_INTERPRETATION_MULTIBAND:
	case 16: // LABQ: a coding this library does not carry
		sane = false;
		break;
	case VIPS_HIP_INTERPRETATION_HISTOGRAM:
		if (width > 1 && height > 1)
			sane = false;
		break;
	case 24: // FOURIER
		if (!format_iscomplex(format))
			sane = false;
		break;
	case VIPS_HIP_INTERPRETATION_scRGB:
	case 23: // YXY
	case 30: // OKLAB
	case 31: // OKLCH
		if (!isfloat)
			sane = false;
		break;
	case VIPS_HIP_INTERPRETATION_LABS:
		if (isuint || is8)
			sane = false;
		break;
	case VIPS_HIP_INTERPRETATION_RGB16:
	case VIPS_HIP_INTERPRETATION_GREY16:
		if (is8)
			sane = false;
		break;
	default:
		break;
	}
	if (sane)
		return type;
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR:
	case VIPS_HIP_FORMAT_SHORT:
	case VIPS_HIP_FORMAT_UINT:
	case VIPS_HIP_FORMAT_INT:
	case VIPS_HIP_FORMAT_FLOAT:
	case VIPS_HIP_FORMAT_DOUBLE:
		return bands <= 2 ? VIPS_HIP_INTERPRETATION_B_W : bands <= 4 ? VIPS_HIP_INTERPRETATION_sRGB : VIPS_HIP_INTERPRETATION_MULTIBAND;
	case VIPS_HIP_FORMAT_USHORT:
		return bands <= 2 ? VIPS_HIP_INTERPRETATION_GREY16 : bands <= 4 ? VIPS_HIP_INTERPRETATION_RGB16 : VIPS_HIP_INTERPRETATION_MULTIBAND;
	case VIPS_HIP_FORMAT_CHAR:
		return bands == 1 ? 27 /* MATRIX */ : VIPS_HIP_INTERPRETATION_MULTIBAND;
	case VIPS_HIP_FORMAT_COMPLEX:
	case VIPS_HIP_FORMAT_DPCOMPLEX:
		return 24; // FOURIER
	default:
		return VIPS_HIP_INTERPRETATION_MULTIBAND;
	}
}

// vips_image_get_format_max, iofuncs/header.c
double vh::format_max(int format)
{
	switch (format) {
	case VIPS_HIP_FORMAT_UCHAR: return UCHAR_MAX;
	case VIPS_HIP_FORMAT_CHAR: return SCHAR_MAX;
	case VIPS_HIP_FORMAT_USHORT: return USHRT_MAX;
	case VIPS_HIP_FORMAT_SHORT: return SHRT_MAX;
	case VIPS_HIP_FORMAT_UINT: return UINT_MAX;
	case VIPS_HIP_FORMAT_INT: return INT_MAX;
	default: return -1;
	}
}

double vh::vips_clip(double lo, double v, double hi)
{
	// VIPS_CLIP
	const double m = hi < v ? hi : v;
	return lo > m ? lo : m;
}

// vips__vector_to_pels (conversion/insert.c:244-334) for one element: vips_linear of a black uchar image makes the
// float, vips_cast (cast.c:123-131, :231-238) clips it as a double and converts
void vh::element_to_format(double real, int format, unsigned char *dst)
{
	const float f = (float) real;
	const double d = (double) f;
	switch (format) {
#define INT_CASE(F, T, LO, HI) \
	case F: { \
		const T v = (T) vips_clip(LO, d, HI); \
		memcpy(dst, &v, sizeof(v)); \
		break; \
	}
		INT_CASE(VIPS_HIP_FORMAT_UCHAR, unsigned char, 0, UCHAR_MAX)
		INT_CASE(VIPS_HIP_FORMAT_CHAR, signed char, SCHAR_MIN, SCHAR_MAX)
		INT_CASE(VIPS_HIP_FORMAT_USHORT, unsigned short, 0, USHRT_MAX)
		INT_CASE(VIPS_HIP_FORMAT_SHORT, short, SHRT_MIN, SHRT_MAX)
		INT_CASE(VIPS_HIP_FORMAT_UINT, unsigned int, 0, UINT_MAX)
		INT_CASE(VIPS_HIP_FORMAT_INT, int, INT_MIN, INT_MAX)
#undef INT_CASE
	case VIPS_HIP_FORMAT_DOUBLE:
		memcpy(dst, &d, sizeof(d));
		break;
	default:
		memcpy(dst, &f, sizeof(f));
		break;
	}
}

// vips_check_noncomplex's words for a complex format
int vh::arithmetic_noncomplex(const char *domain, int format)
{
	if (format_iscomplex(format)) {
		error(domain, "image must be non-complex");
		return -1;
	}
	if (format_sizeof(format) == 0) {
		error(domain, "unknown band format %d", format);
		return -1;
	}
	return 0;
}
